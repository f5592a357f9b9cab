"""CPU: the C ABI of the per-base qualities (csrc/wn_quality.hip): the exported symbol, the ctypes row against the header, and
the shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls below touches a device."""

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, check_row, header_names

NAME = "wn_ctc_base_quality"
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_quality_symbol_is_exported(lib):
    from wavenet_speech_amd import _lib
    assert NAME in _lib.SIGNATURES
    assert hasattr(lib, NAME)
    assert lib.wn_version() == 300                                   # an additive entry point


def test_signature_row_matches_the_header():
    check_row(NAME, count=25, opaque=True)
    names = header_names(NAME)
    assert names == ["x", "sb", "sc", "st", "input_kind", "input_lengths", "labels", "labels_stride", "frames", "frames_stride",
                     "lengths", "batch", "classes", "length", "max_labels", "blank", "stat", "qscale", "qbias", "error", "qual",
                     "dwell", "read_error", "bad", "stream"]


def _call(lib, x=FAKE, strides=(500, 100, 1), input_kind=0, input_lengths=None, labels=FAKE, labels_stride=100, frames=FAKE,
          frames_stride=100, lengths=FAKE, batch=2, classes=5, length=100, max_labels=100, blank=0, stat=0, qscale=1.0, qbias=0.0,
          error=FAKE, qual=FAKE, dwell=FAKE, read_error=FAKE, bad=None):
    return lib.wn_ctc_base_quality(x, strides[0], strides[1], strides[2], input_kind, input_lengths, labels, labels_stride, frames,
                                   frames_stride, lengths, batch, classes, length, max_labels, blank, stat, qscale, qbias, error, qual,
                                   dwell, read_error, bad, None)


def test_rejects_on_the_host(lib):
    for kw in (dict(batch=0), dict(batch=-1), dict(length=0), dict(length=-5), dict(max_labels=0), dict(max_labels=-1),
               dict(classes=1), dict(classes=0), dict(classes=-3), dict(labels_stride=-1), dict(frames_stride=-100),
               dict(input_kind=-1), dict(input_kind=3), dict(stat=-1), dict(stat=2), dict(qscale=0.0), dict(qscale=-1.0),
               dict(qscale=INF), dict(qscale=NAN), dict(qbias=INF), dict(qbias=-INF), dict(qbias=NAN)):
        assert _call(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    assert _call(lib, classes=65) == WN_ERR_UNSUPPORTED
    assert _call(lib, length=2 ** 24 + 1) == WN_ERR_UNSUPPORTED
    assert _call(lib, max_labels=101) == WN_ERR_UNSUPPORTED          # more labels than frames
    assert _call(lib, batch=65536) == WN_ERR_UNSUPPORTED
    # a launch stays below 2^32 threads: 256 * ceil(max_labels / 256) * batch
    assert _call(lib, length=2 ** 24, max_labels=2 ** 24, batch=256) == WN_ERR_UNSUPPORTED              # 2^32
    assert _call(lib, length=2 ** 24, max_labels=2 ** 24 - 255, batch=256) == WN_ERR_UNSUPPORTED         # rounds up to 2^32
    # the accepted side of each limit goes on to the pointer checks
    assert _call(lib, classes=64, x=None) == WN_ERR_NULL
    assert _call(lib, classes=2, x=None) == WN_ERR_NULL
    assert _call(lib, length=2 ** 24, x=None) == WN_ERR_NULL
    assert _call(lib, max_labels=100, length=100, x=None) == WN_ERR_NULL
    assert _call(lib, max_labels=1, length=1, batch=1, x=None) == WN_ERR_NULL
    assert _call(lib, batch=65535, x=None) == WN_ERR_NULL
    assert _call(lib, length=2 ** 24, max_labels=2 ** 24, batch=255, x=None) == WN_ERR_NULL             # 2^32 - 2^24
    assert _call(lib, length=2 ** 24, max_labels=2 ** 24 - 256, batch=256, x=None) == WN_ERR_NULL        # 2^32 - 2^16
    assert _call(lib, labels_stride=0, frames_stride=0, x=None) == WN_ERR_NULL           # one row for every read is a valid layout
    assert _call(lib, blank=-1, x=None) == WN_ERR_NULL               # a blank no label can equal: left to the caller
    for kw in (dict(input_kind=2), dict(stat=1), dict(qscale=1e-30), dict(qscale=3e38), dict(qbias=-3e38)):
        assert _call(lib, x=None, **kw) == WN_ERR_NULL, kw
    for name in ("x", "labels", "frames", "lengths"):                # input_lengths and bad are optional (NULL in every call here)
        assert _call(lib, **{name: None}) == WN_ERR_NULL, name
    assert _call(lib, error=None, qual=None, dwell=None, read_error=None) == WN_ERR_NULL                # nothing to compute
    assert _call(lib, error=None, qual=None, dwell=None, read_error=None, bad=FAKE) == WN_ERR_NULL      # the flag is no output
    # the order of the checks: shape, then unsupported, then NULL
    assert _call(lib, batch=0, classes=65, x=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, qscale=NAN, length=2 ** 24 + 1, labels=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, stat=2, batch=65536, x=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, classes=65, x=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, max_labels=101, error=None, qual=None, dwell=None, read_error=None) == WN_ERR_UNSUPPORTED
