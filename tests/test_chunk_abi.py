"""CPU: the C ABI of chunked inference (csrc/wn_chunk.hip): exported symbols, the ctypes table against the header, and the
shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls below touches a device."""
import ctypes

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, check_row

NAMES = ("wn_chunk_gather", "wn_chunk_stitch")
EDGE = 2 ** 31 - 1024                    # the first ld / chunk / frame count that is refused


@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_chunk_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.wn_version() == 300                                   # additive entry points


def test_signature_table_matches_the_header():
    for name in NAMES:
        check_row(name, opaque=True)


def _gather(lib, signal=FAKE, is_int16=0, batch=2, ld=100, signal_lengths=FAKE, scale=None, shift=None, plan=FAKE, n_chunks=3, chunk=32,
            out=FAKE, bad=None):
    return lib.wn_chunk_gather(signal, is_int16, batch, ld, signal_lengths, scale, shift, plan, n_chunks, chunk, out, bad, None)


def test_chunk_gather_rejects_on_the_host(lib):
    for kw in (dict(batch=0), dict(batch=-1), dict(ld=0), dict(ld=-7), dict(n_chunks=0), dict(n_chunks=-3), dict(chunk=0), dict(chunk=-4),
               dict(chunk=30), dict(chunk=33), dict(chunk=2)):
        assert _gather(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    assert _gather(lib, n_chunks=65536) == WN_ERR_UNSUPPORTED
    assert _gather(lib, ld=EDGE) == WN_ERR_UNSUPPORTED
    assert _gather(lib, chunk=EDGE) == WN_ERR_UNSUPPORTED            # 2^31 - 1024 is a multiple of 4: the limit, not the shape
    # the accepted side of each edge goes on to the pointer checks
    assert _gather(lib, n_chunks=65535, out=None) == WN_ERR_NULL
    assert _gather(lib, ld=EDGE - 1, out=None) == WN_ERR_NULL
    assert _gather(lib, chunk=EDGE - 4, out=None) == WN_ERR_NULL
    assert _gather(lib, chunk=4, out=None) == WN_ERR_NULL
    # a launch stays below 2^32 threads: 256 * ceil(chunk / 1024) * n_chunks
    assert _gather(lib, chunk=1024 * 256, n_chunks=65535, out=None) == WN_ERR_NULL                      # 2^32 - 2^16
    assert _gather(lib, chunk=1024 * 512, n_chunks=32768) == WN_ERR_UNSUPPORTED                         # 2^32
    for is_int16 in (0, 1):
        for name in ("signal", "signal_lengths", "plan", "out"):     # scale, shift and bad are optional (NULL in every call here)
            assert _gather(lib, is_int16=is_int16, **{name: None}) == WN_ERR_NULL, name
    assert _gather(lib, out=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE          # rows are stored 16 bytes at a time
    assert _gather(lib, out=ctypes.c_void_p((1 << 20) + 4)) == WN_ERR_WORKSPACE
    # the order of the checks: shape, then unsupported, then NULL, then alignment
    assert _gather(lib, chunk=30, n_chunks=65536, plan=None) == WN_ERR_BAD_SHAPE
    assert _gather(lib, batch=0, ld=EDGE, plan=None) == WN_ERR_BAD_SHAPE
    assert _gather(lib, n_chunks=65536, plan=None, out=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_UNSUPPORTED
    assert _gather(lib, plan=None, out=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_NULL


def _stitch(lib, y=FAKE, strides=(5 * 34, 34, 1), y_frames=34, plan=FAKE, n_chunks=3, classes=5, batch=2, out=FAKE, out_strides=(500, 100),
            out_frames=100, frame_lengths=FAKE, bad=None):
    return lib.wn_chunk_stitch(y, strides[0], strides[1], strides[2], y_frames, plan, n_chunks, classes, batch, out, out_strides[0],
                               out_strides[1], out_frames, frame_lengths, bad, None)


def test_chunk_stitch_rejects_on_the_host(lib):
    for kw in (dict(batch=0), dict(n_chunks=0), dict(n_chunks=-1), dict(classes=0), dict(classes=-5), dict(y_frames=0), dict(out_frames=0),
               dict(out_frames=-2), dict(strides=(-1, 34, 1)), dict(strides=(170, -34, 1)), dict(strides=(170, 34, -1)),
               dict(out_strides=(-500, 100)), dict(out_strides=(500, -100))):
        assert _stitch(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    assert _stitch(lib, n_chunks=65536) == WN_ERR_UNSUPPORTED
    assert _stitch(lib, classes=65536) == WN_ERR_UNSUPPORTED
    assert _stitch(lib, y_frames=EDGE) == WN_ERR_UNSUPPORTED
    assert _stitch(lib, out_frames=EDGE) == WN_ERR_UNSUPPORTED
    assert _stitch(lib, n_chunks=65535, out=None) == WN_ERR_NULL
    assert _stitch(lib, classes=65535, out=None) == WN_ERR_NULL
    assert _stitch(lib, y_frames=EDGE - 1, classes=1, n_chunks=1, out=None) == WN_ERR_NULL
    # a launch stays below 2^32 threads: 256 * ceil(y_frames / 256) * classes * n_chunks
    assert _stitch(lib, y_frames=256, classes=256, n_chunks=65535, out=None) == WN_ERR_NULL             # 2^32 - 2^16
    assert _stitch(lib, y_frames=257, classes=256, n_chunks=32768) == WN_ERR_UNSUPPORTED                # 2^32
    assert _stitch(lib, y_frames=256, classes=65535, n_chunks=65535) == WN_ERR_UNSUPPORTED
    assert _stitch(lib, out_frames=EDGE - 1, out=None) == WN_ERR_NULL
    assert _stitch(lib, strides=(0, 0, 0), out=None) == WN_ERR_NULL                       # a broadcast y is a valid layout
    for name in ("y", "plan", "out", "frame_lengths"):                                   # bad is optional
        assert _stitch(lib, **{name: None}) == WN_ERR_NULL, name
    # the order of the checks: shape, then unsupported, then NULL
    assert _stitch(lib, classes=0, n_chunks=65536, y=None) == WN_ERR_BAD_SHAPE
    assert _stitch(lib, strides=(170, 34, -1), y_frames=EDGE, y=None) == WN_ERR_BAD_SHAPE
    assert _stitch(lib, n_chunks=65536, y=None) == WN_ERR_UNSUPPORTED
