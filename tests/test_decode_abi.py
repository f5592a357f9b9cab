"""CPU: the C ABI of the CTC decoders (csrc/wn_decode.hip): exported symbols, workspace sizes, and the shape / limit / pointer
checks, which run on the host before any HIP call -- none of the calls below touches a device."""
import ctypes

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE



@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_decode_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for name in ("wn_ctc_decode_workspace_bytes", "wn_ctc_greedy_decode", "wn_ctc_beam_decode"):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)


def test_workspace_bytes(lib):
    for B, C, T, W in [(1, 2, 1, 1), (8, 5, 1000, 8), (32, 5, 4096, 64), (2, 64, 100, 64)]:
        n = lib.wn_ctc_decode_workspace_bytes(B, C, T, W)
        assert n >= B * T * W * 8 and n % 16 == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 5, 1000, 0) == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 5, 1000, 65) == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 65, 1000, 8) == 0
    assert lib.wn_ctc_decode_workspace_bytes(0, 5, 1000, 8) == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 1, 1000, 8) == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 5, 0, 8) == 0


def _beam(lib, B=2, C=5, T=10, W=4, kind=0, ptr=FAKE, ws=FAKE, ws_bytes=1 << 30):
    return lib.wn_ctc_beam_decode(ptr, C * T, T, 1, kind, None, B, C, T, 0, W, ptr, None, ptr, ptr, ws, ws_bytes, None, None)


def test_beam_decode_rejects_on_the_host(lib):
    assert _beam(lib, C=65) == WN_ERR_UNSUPPORTED
    assert _beam(lib, W=65) == WN_ERR_UNSUPPORTED
    assert _beam(lib, W=0) == WN_ERR_BAD_SHAPE
    assert _beam(lib, B=0) == WN_ERR_BAD_SHAPE
    assert _beam(lib, C=1) == WN_ERR_BAD_SHAPE
    assert _beam(lib, T=0) == WN_ERR_BAD_SHAPE
    assert _beam(lib, kind=3) == WN_ERR_BAD_SHAPE
    assert _beam(lib, ptr=None) == WN_ERR_NULL
    assert _beam(lib, ws=None) == WN_ERR_NULL
    assert _beam(lib, ws_bytes=16) == WN_ERR_WORKSPACE
    assert _beam(lib, ws=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE      # not 16-byte aligned


def test_greedy_decode_rejects_on_the_host(lib):
    def greedy(B=2, C=5, T=10, ptr=FAKE):
        return lib.wn_ctc_greedy_decode(ptr, C * T, T, 1, None, B, C, T, 0, ptr, None, ptr, None, None)
    assert greedy(C=65) == WN_ERR_UNSUPPORTED
    assert greedy(C=1) == WN_ERR_BAD_SHAPE
    assert greedy(B=0) == WN_ERR_BAD_SHAPE
    assert greedy(T=0) == WN_ERR_BAD_SHAPE
    assert greedy(ptr=None) == WN_ERR_NULL
