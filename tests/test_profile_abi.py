"""CPU: the C ABI of the quality profile (csrc/wn_profile.hip): the exported symbol, the ctypes row against the header, and the
shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls below touches a device."""

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, check_row, header_names

NAME = "wn_quality_profile"
OUTPUTS = ("q_counts", "dwell_counts", "confusion", "read_counts", "outcome", "ref_index")


@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_profile_symbol_is_exported(lib):
    from wavenet_speech_amd import _lib
    assert NAME in _lib.SIGNATURES
    assert hasattr(lib, NAME)
    assert lib.wn_version() == 300                                   # an additive entry point


def test_signature_row_matches_the_header():
    check_row(NAME, count=27, opaque=True)
    names = header_names(NAME)
    assert names == ["ops", "ops_stride", "ops_len", "ref", "ref_stride", "ref_lengths", "query", "query_stride", "query_lengths",
                     "qual", "qual_stride", "dwell", "dwell_stride", "batch", "max_ref_len", "max_query_len", "max_ops", "classes",
                     "count_ends", "q_counts", "dwell_counts", "confusion", "read_counts", "outcome", "ref_index", "bad", "stream"]


def _call(lib, ops=FAKE, ops_stride=200, ops_len=FAKE, ref=FAKE, ref_stride=100, ref_lengths=FAKE, query=FAKE, query_stride=100,
          query_lengths=FAKE, qual=FAKE, qual_stride=100, dwell=FAKE, dwell_stride=100, batch=2, max_ref_len=100, max_query_len=100,
          max_ops=200, classes=5, count_ends=0, q_counts=FAKE, dwell_counts=FAKE, confusion=FAKE, read_counts=FAKE, outcome=FAKE,
          ref_index=FAKE, bad=None):
    return lib.wn_quality_profile(ops, ops_stride, ops_len, ref, ref_stride, ref_lengths, query, query_stride, query_lengths, qual,
                                  qual_stride, dwell, dwell_stride, batch, max_ref_len, max_query_len, max_ops, classes, count_ends,
                                  q_counts, dwell_counts, confusion, read_counts, outcome, ref_index, bad, None)


def test_rejects_on_the_host(lib):
    for kw in (dict(batch=0), dict(batch=-1), dict(max_ref_len=0), dict(max_ref_len=-7), dict(max_query_len=0),
               dict(max_query_len=-1), dict(max_ops=0), dict(max_ops=-200), dict(classes=0), dict(classes=-5),
               dict(ops_stride=-1), dict(ref_stride=-1), dict(query_stride=-100), dict(qual_stride=-1), dict(dwell_stride=-1),
               dict(count_ends=-1), dict(count_ends=2)):
        assert _call(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    assert _call(lib, classes=65) == WN_ERR_UNSUPPORTED
    assert _call(lib, max_query_len=8193, max_ops=8193) == WN_ERR_UNSUPPORTED
    assert _call(lib, max_ref_len=65536) == WN_ERR_UNSUPPORTED
    assert _call(lib, max_ops=201) == WN_ERR_UNSUPPORTED             # more columns than labels
    assert _call(lib, max_ref_len=65535, max_query_len=8192, max_ops=65535 + 8192 + 1) == WN_ERR_UNSUPPORTED
    assert _call(lib, batch=65536) == WN_ERR_UNSUPPORTED
    # the accepted side of each limit goes on to the pointer checks
    for kw in (dict(classes=64), dict(classes=1), dict(max_query_len=8192), dict(max_query_len=1, max_ops=101),
               dict(max_ref_len=65535), dict(max_ref_len=1, max_ops=101), dict(max_ops=200), dict(max_ops=1),
               dict(max_ref_len=65535, max_query_len=8192, max_ops=65535 + 8192), dict(batch=65535), dict(batch=1),
               dict(count_ends=1), dict(ops_stride=0, ref_stride=0, query_stride=0, qual_stride=0, dwell_stride=0)):
        assert _call(lib, ops=None, **kw) == WN_ERR_NULL, kw
    for name in ("ops", "ops_len", "ref", "ref_lengths", "query", "query_lengths"):
        assert _call(lib, **{name: None}) == WN_ERR_NULL, name
    # a table and its input come together
    assert _call(lib, qual=None) == WN_ERR_NULL and _call(lib, q_counts=None) == WN_ERR_NULL
    assert _call(lib, dwell=None) == WN_ERR_NULL and _call(lib, dwell_counts=None) == WN_ERR_NULL
    nothing = dict(qual=None, dwell=None, **{name: None for name in OUTPUTS})
    assert _call(lib, **nothing) == WN_ERR_NULL                      # nothing to compute
    assert _call(lib, bad=FAKE, **nothing) == WN_ERR_NULL            # the flag is no output
    # the order of the checks: shape, then unsupported, then NULL
    assert _call(lib, batch=0, classes=65, ops=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, count_ends=2, max_ref_len=65536, ref=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, qual_stride=-1, batch=65536, **nothing) == WN_ERR_BAD_SHAPE
    assert _call(lib, classes=65, ops=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, max_ops=201, **nothing) == WN_ERR_UNSUPPORTED
    assert _call(lib, batch=65536, qual=None) == WN_ERR_UNSUPPORTED
