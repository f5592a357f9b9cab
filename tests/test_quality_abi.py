"""CPU: the C ABI of the per-base qualities (csrc/wn_quality.hip): the exported symbol, the ctypes row against the header, and
the shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls below touches a device."""
from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, Entry
from tests.abi_util import lib  # noqa: F401

QUALITY = Entry("wn_ctc_base_quality", dict(x=FAKE, sb=500, sc=100, st=1, input_kind=0, input_lengths=None, labels=FAKE, labels_stride=100, frames=FAKE,
                                            frames_stride=100, lengths=FAKE, batch=2, classes=5, length=100, max_labels=100, blank=0, stat=0,
                                            qscale=1.0, qbias=0.0, error=FAKE, qual=FAKE, dwell=FAKE, read_error=FAKE, bad=None, stream=None))
INF, NAN = float("inf"), float("nan")


def test_quality_symbol_is_exported(lib):
    QUALITY.check_exported(lib)


def test_signature_row_matches_the_header():
    QUALITY.check_declared()                                         # 25 arguments


def test_rejects_on_the_host(lib):
    QUALITY.rejects(lib, "x",
                    shape=(dict(batch=0), dict(batch=-1), dict(length=0), dict(length=-5), dict(max_labels=0), dict(max_labels=-1),
                           dict(classes=1), dict(classes=0), dict(classes=-3), dict(labels_stride=-1), dict(frames_stride=-100),
                           dict(input_kind=-1), dict(input_kind=3), dict(stat=-1), dict(stat=2), dict(qscale=0.0), dict(qscale=-1.0),
                           dict(qscale=INF), dict(qscale=NAN), dict(qbias=INF), dict(qbias=-INF), dict(qbias=NAN)),
                    unsupported=(dict(classes=65), dict(length=2 ** 24 + 1), dict(batch=65536),
                                 dict(max_labels=101),                                         # more labels than frames
                                 # a launch stays below 2^32 threads: 256 * ceil(max_labels / 256) * batch
                                 dict(length=2 ** 24, max_labels=2 ** 24, batch=256),          # 2^32
                                 dict(length=2 ** 24, max_labels=2 ** 24 - 255, batch=256)),   # rounds up to 2^32
                    accepted=(dict(classes=64), dict(classes=2), dict(length=2 ** 24), dict(max_labels=100, length=100),
                              dict(max_labels=1, length=1, batch=1), dict(batch=65535),
                              dict(length=2 ** 24, max_labels=2 ** 24, batch=255),             # 2^32 - 2^24
                              dict(length=2 ** 24, max_labels=2 ** 24 - 256, batch=256),       # 2^32 - 2^16
                              dict(labels_stride=0, frames_stride=0),                          # one row for every read is a valid layout
                              dict(blank=-1),                                                  # a blank no label can equal: left to the caller
                              dict(input_kind=2), dict(stat=1), dict(qscale=1e-30), dict(qscale=3e38), dict(qbias=-3e38)),
                    required=("x", "labels", "frames", "lengths"))   # input_lengths and bad are optional (NULL in every call here)
    assert QUALITY(lib, error=None, qual=None, dwell=None, read_error=None) == WN_ERR_NULL              # nothing to compute
    assert QUALITY(lib, error=None, qual=None, dwell=None, read_error=None, bad=FAKE) == WN_ERR_NULL    # the flag is no output
    # the order of the checks: shape, then unsupported, then NULL
    assert QUALITY(lib, batch=0, classes=65, x=None) == WN_ERR_BAD_SHAPE
    assert QUALITY(lib, qscale=NAN, length=2 ** 24 + 1, labels=None) == WN_ERR_BAD_SHAPE
    assert QUALITY(lib, stat=2, batch=65536, x=None) == WN_ERR_BAD_SHAPE
    assert QUALITY(lib, classes=65, x=None) == WN_ERR_UNSUPPORTED
    assert QUALITY(lib, max_labels=101, error=None, qual=None, dwell=None, read_error=None) == WN_ERR_UNSUPPORTED
