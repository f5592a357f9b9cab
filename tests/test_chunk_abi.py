"""CPU: the C ABI of chunked inference (csrc/wn_chunk.hip): exported symbols, the ctypes table against the header, and the
shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls below touches a device."""
import ctypes

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

GATHER = Entry("wn_chunk_gather", dict(signal=FAKE, signal_is_int16=0, batch=2, ld=100, signal_lengths=FAKE, scale=None, shift=None, plan=FAKE,
                                       n_chunks=3, chunk=32, out=FAKE, bad=None, stream=None))
STITCH = Entry("wn_chunk_stitch", dict(y=FAKE, stride_n=5 * 34, stride_c=34, stride_t=1, y_frames=34, plan=FAKE, n_chunks=3, classes=5, batch=2,
                                       out=FAKE, out_stride_b=500, out_stride_c=100, out_frames=100, frame_lengths=FAKE, bad=None, stream=None))
EDGE = 2 ** 31 - 1024                    # the first ld / chunk / frame count that is refused
GATHER_REQUIRED = ("signal", "signal_lengths", "plan", "out")        # scale, shift and bad are optional (NULL in every call here)


def test_chunk_symbols_are_exported(lib):
    GATHER.check_exported(lib)
    STITCH.check_exported(lib)


def test_signature_table_matches_the_header():
    GATHER.check_declared()                                          # 13 arguments
    STITCH.check_declared()                                          # 16


def test_chunk_gather_rejects_on_the_host(lib):
    GATHER.rejects(lib, "out",
                   shape=(dict(batch=0), dict(batch=-1), dict(ld=0), dict(ld=-7), dict(n_chunks=0), dict(n_chunks=-3), dict(chunk=0),
                          dict(chunk=-4), dict(chunk=30), dict(chunk=33), dict(chunk=2)),
                   unsupported=(dict(n_chunks=65536), dict(ld=EDGE),
                                dict(chunk=EDGE),                    # 2^31 - 1024 is a multiple of 4: the limit, not the shape
                                # a launch stays below 2^32 threads: 256 * ceil(chunk / 1024) * n_chunks
                                dict(chunk=1024 * 512, n_chunks=32768)),                       # 2^32
                   accepted=(dict(n_chunks=65535), dict(ld=EDGE - 1), dict(chunk=EDGE - 4), dict(chunk=4),
                             dict(chunk=1024 * 256, n_chunks=65535)),                          # 2^32 - 2^16
                   required=GATHER_REQUIRED)
    for name in GATHER_REQUIRED:
        assert GATHER(lib, signal_is_int16=1, **{name: None}) == WN_ERR_NULL, name
    assert GATHER(lib, out=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE           # rows are stored 16 bytes at a time
    assert GATHER(lib, out=ctypes.c_void_p((1 << 20) + 4)) == WN_ERR_WORKSPACE
    # the order of the checks: shape, then unsupported, then NULL, then alignment
    assert GATHER(lib, chunk=30, n_chunks=65536, plan=None) == WN_ERR_BAD_SHAPE
    assert GATHER(lib, batch=0, ld=EDGE, plan=None) == WN_ERR_BAD_SHAPE
    assert GATHER(lib, n_chunks=65536, plan=None, out=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_UNSUPPORTED
    assert GATHER(lib, plan=None, out=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_NULL


def test_chunk_stitch_rejects_on_the_host(lib):
    STITCH.rejects(lib, "out",
                   shape=(dict(batch=0), dict(n_chunks=0), dict(n_chunks=-1), dict(classes=0), dict(classes=-5), dict(y_frames=0),
                          dict(out_frames=0), dict(out_frames=-2), dict(stride_n=-1), dict(stride_c=-34), dict(stride_t=-1),
                          dict(out_stride_b=-500), dict(out_stride_c=-100)),
                   unsupported=(dict(n_chunks=65536), dict(classes=65536), dict(y_frames=EDGE), dict(out_frames=EDGE),
                                # a launch stays below 2^32 threads: 256 * ceil(y_frames / 256) * classes * n_chunks
                                dict(y_frames=257, classes=256, n_chunks=32768),               # 2^32
                                dict(y_frames=256, classes=65535, n_chunks=65535)),
                   accepted=(dict(n_chunks=65535), dict(classes=65535), dict(y_frames=EDGE - 1, classes=1, n_chunks=1),
                             dict(y_frames=256, classes=256, n_chunks=65535),                  # 2^32 - 2^16
                             dict(out_frames=EDGE - 1),
                             dict(stride_n=0, stride_c=0, stride_t=0)),                        # a broadcast y is a valid layout
                   required=("y", "plan", "out", "frame_lengths"))                             # bad is optional
    # the order of the checks: shape, then unsupported, then NULL
    assert STITCH(lib, classes=0, n_chunks=65536, y=None) == WN_ERR_BAD_SHAPE
    assert STITCH(lib, stride_t=-1, y_frames=EDGE, y=None) == WN_ERR_BAD_SHAPE
    assert STITCH(lib, n_chunks=65536, y=None) == WN_ERR_UNSUPPORTED
