"""CPU: the C ABI of the quality profile (csrc/wn_profile.hip): the exported symbol, the ctypes row against the header, and the
shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls below touches a device."""
from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, Entry
from tests.abi_util import lib  # noqa: F401

PROFILE = Entry("wn_quality_profile", dict(ops=FAKE, ops_stride=200, ops_len=FAKE, ref=FAKE, ref_stride=100, ref_lengths=FAKE, query=FAKE,
                                           query_stride=100, query_lengths=FAKE, qual=FAKE, qual_stride=100, dwell=FAKE, dwell_stride=100, batch=2,
                                           max_ref_len=100, max_query_len=100, max_ops=200, classes=5, count_ends=0, q_counts=FAKE,
                                           dwell_counts=FAKE, confusion=FAKE, read_counts=FAKE, outcome=FAKE, ref_index=FAKE, bad=None, stream=None))
OUTPUTS = ("q_counts", "dwell_counts", "confusion", "read_counts", "outcome", "ref_index")


def test_profile_symbol_is_exported(lib):
    PROFILE.check_exported(lib)


def test_signature_row_matches_the_header():
    PROFILE.check_declared()                                         # 27 arguments


def test_rejects_on_the_host(lib):
    PROFILE.rejects(lib, "ops",
                    shape=(dict(batch=0), dict(batch=-1), dict(max_ref_len=0), dict(max_ref_len=-7), dict(max_query_len=0),
                           dict(max_query_len=-1), dict(max_ops=0), dict(max_ops=-200), dict(classes=0), dict(classes=-5),
                           dict(ops_stride=-1), dict(ref_stride=-1), dict(query_stride=-100), dict(qual_stride=-1), dict(dwell_stride=-1),
                           dict(count_ends=-1), dict(count_ends=2)),
                    unsupported=(dict(classes=65), dict(max_query_len=8193, max_ops=8193), dict(max_ref_len=65536),
                                 dict(max_ops=201),                  # more columns than labels
                                 dict(max_ref_len=65535, max_query_len=8192, max_ops=65535 + 8192 + 1), dict(batch=65536)),
                    accepted=(dict(classes=64), dict(classes=1), dict(max_query_len=8192), dict(max_query_len=1, max_ops=101),
                              dict(max_ref_len=65535), dict(max_ref_len=1, max_ops=101), dict(max_ops=200), dict(max_ops=1),
                              dict(max_ref_len=65535, max_query_len=8192, max_ops=65535 + 8192), dict(batch=65535), dict(batch=1),
                              dict(count_ends=1), dict(ops_stride=0, ref_stride=0, query_stride=0, qual_stride=0, dwell_stride=0)),
                    required=("ops", "ops_len", "ref", "ref_lengths", "query", "query_lengths"))
    # a table and its input come together
    assert PROFILE(lib, qual=None) == WN_ERR_NULL and PROFILE(lib, q_counts=None) == WN_ERR_NULL
    assert PROFILE(lib, dwell=None) == WN_ERR_NULL and PROFILE(lib, dwell_counts=None) == WN_ERR_NULL
    nothing = dict(qual=None, dwell=None, **{name: None for name in OUTPUTS})
    assert PROFILE(lib, **nothing) == WN_ERR_NULL                    # nothing to compute
    assert PROFILE(lib, bad=FAKE, **nothing) == WN_ERR_NULL          # the flag is no output
    # the order of the checks: shape, then unsupported, then NULL
    assert PROFILE(lib, batch=0, classes=65, ops=None) == WN_ERR_BAD_SHAPE
    assert PROFILE(lib, count_ends=2, max_ref_len=65536, ref=None) == WN_ERR_BAD_SHAPE
    assert PROFILE(lib, qual_stride=-1, batch=65536, **nothing) == WN_ERR_BAD_SHAPE
    assert PROFILE(lib, classes=65, ops=None) == WN_ERR_UNSUPPORTED
    assert PROFILE(lib, max_ops=201, **nothing) == WN_ERR_UNSUPPORTED
    assert PROFILE(lib, batch=65536, qual=None) == WN_ERR_UNSUPPORTED
