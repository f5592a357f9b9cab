"""CPU: the C ABI of CTC forced alignment (csrc/wn_align.hip): exported symbols, workspace sizes, and the shape / limit /
pointer checks, which run on the host before any HIP call -- none of the calls below touches a device."""
import ctypes

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE



@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_align_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for name in ("wn_ctc_align_workspace_bytes", "wn_ctc_align"):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.wn_version() == 300


def test_workspace_bytes(lib):
    for B, C, T, L in [(1, 2, 1, 1), (8, 5, 1000, 100), (32, 5, 4096, 410), (8, 5, 4096, 2047), (2, 64, 100, 31), (3, 5, 77, 32)]:
        n = lib.wn_ctc_align_workspace_bytes(B, C, T, L)
        sp = (2 * L + 1 + 63) // 64 * 64
        assert n % 16 == 0
        assert n >= B * T * ((2 * L + 1 + 3) // 4)                   # 2 bits per state and frame
        assert n <= B * T * (sp + 16) + 256                          # the loss takes 16 bytes per state and frame
        assert n <= lib.wn_ctc_workspace_bytes(B, C, T, L) // 16
    for B, C, T, L in [(0, 5, 100, 10), (8, 1, 100, 10), (8, 5, 0, 10), (8, 5, 100, 0), (-1, 5, 100, 10), (8, 5, 100, -3),
                       (8, 65, 100, 10), (8, 5, 100, 2048), (8, 5, (1 << 24) + 1, 10), (65536, 5, 100, 10),
                       (65535, 5, 1 << 16, 10)]:
        assert lib.wn_ctc_align_workspace_bytes(B, C, T, L) == 0, (B, C, T, L)


def _align(lib, B=2, C=5, T=10, L=4, kind=0, blank=0, x=FAKE, labels=FAKE, label_len=FAKE, states=FAKE, score=FAKE, ws=FAKE,
           ws_bytes=1 << 30):
    return lib.wn_ctc_align(x, C * T, T, 1, kind, labels, label_len, None, B, C, T, L, blank, states, None, None, score, ws,
                            ws_bytes, None, None)


def test_align_rejects_on_the_host(lib):
    assert _align(lib, C=65) == WN_ERR_UNSUPPORTED
    assert _align(lib, L=2048) == WN_ERR_UNSUPPORTED
    assert _align(lib, T=(1 << 24) + 1) == WN_ERR_UNSUPPORTED
    assert _align(lib, B=65536) == WN_ERR_UNSUPPORTED
    assert _align(lib, B=0) == WN_ERR_BAD_SHAPE
    assert _align(lib, C=1) == WN_ERR_BAD_SHAPE
    assert _align(lib, T=0) == WN_ERR_BAD_SHAPE
    assert _align(lib, L=0) == WN_ERR_BAD_SHAPE
    assert _align(lib, kind=3) == WN_ERR_BAD_SHAPE
    assert _align(lib, kind=-1) == WN_ERR_BAD_SHAPE
    assert _align(lib, blank=5) == WN_ERR_BAD_SHAPE
    assert _align(lib, blank=-1) == WN_ERR_BAD_SHAPE
    for name in ("x", "labels", "label_len", "states", "score", "ws"):
        assert _align(lib, **{name: None}) == WN_ERR_NULL, name
    need = lib.wn_ctc_align_workspace_bytes(2, 5, 10, 4)
    assert need > 0
    assert _align(lib, ws_bytes=need - 1) == WN_ERR_WORKSPACE
    assert _align(lib, ws_bytes=0) == WN_ERR_WORKSPACE
    assert _align(lib, ws=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE      # not 16-byte aligned
    # the order of the checks: shape, then unsupported, then NULL, then workspace
    assert _align(lib, B=0, C=65, x=None) == WN_ERR_BAD_SHAPE
    assert _align(lib, C=65, x=None, ws_bytes=0) == WN_ERR_UNSUPPORTED
    assert _align(lib, x=None, ws_bytes=0) == WN_ERR_NULL
