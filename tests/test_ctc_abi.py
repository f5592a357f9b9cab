"""CPU: the C ABI of the CTC loss (csrc/wn_ctc.hip): exported symbols, the workspace size, and the shape / limit / pointer /
workspace checks, which run on the host before any HIP call -- none of the calls below touches a device."""
import ctypes
import os
import re

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE

MAX_CLASSES, MAX_LABELS, MAX_BATCH = 64, 2047, 65535


@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_ctc_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for name in ("wn_ctc_workspace_bytes", "wn_ctc_loss"):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["wn_ctc_loss"][1]) == 15 and len(_lib.SIGNATURES["wn_ctc_workspace_bytes"][1]) == 4


def _bytes(B, T, L):
    sp = (2 * L + 1 + 63) // 64 * 64
    return B * T * 8 + 2 * B * T * sp * 8 + B * 8 + 256


def test_workspace_bytes(lib):
    for B, C, T, L in [(1, 2, 1, 1), (3, 5, 77, 31), (3, 5, 77, 32), (8, 5, 1000, 100), (32, 5, 4098, 420), (1, 64, 2304, 2047),
                       (2, MAX_CLASSES, 100, 31), (2, 5, 100, MAX_LABELS), (MAX_BATCH, 5, 100, 10), (MAX_BATCH, 5, 32768, 1)]:
        assert lib.wn_ctc_workspace_bytes(B, C, T, L) == _bytes(B, T, L), (B, C, T, L)
    assert _bytes(1, 2304, 2047) == 151_013_640                          # the 151 MB of the 2047-label test
    for B, C, T, L in [(0, 5, 100, 10), (8, 1, 100, 10), (8, 0, 100, 10), (8, 5, 0, 10), (8, 5, 100, 0), (-1, 5, 100, 10), (8, -5, 100, 10),
                       (8, 5, -100, 10), (8, 5, 100, -3), (8, MAX_CLASSES + 1, 100, 10), (8, 5, 100, MAX_LABELS + 1),
                       (MAX_BATCH + 1, 5, 100, 10), (MAX_BATCH, 5, 32769, 10), (2, 5, 2 ** 30, 10)]:
        assert lib.wn_ctc_workspace_bytes(B, C, T, L) == 0, (B, C, T, L)


def _loss(lib, B=2, C=5, T=10, L=4, blank=0, x=FAKE, labels=FAKE, label_len=FAKE, in_len=None, nll=FAKE, dx=FAKE, ws=FAKE,
          ws_bytes=1 << 40, bad=None):
    return lib.wn_ctc_loss(x, labels, label_len, in_len, B, C, T, L, blank, nll, dx, ws, ws_bytes, bad, None)


def test_loss_rejects_on_the_host(lib):
    for kw in (dict(B=0), dict(B=-2), dict(C=1), dict(C=0), dict(T=0), dict(T=-1), dict(L=0), dict(L=-1), dict(blank=5), dict(blank=-1),
               dict(C=64, blank=64)):
        assert _loss(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    for kw in (dict(C=MAX_CLASSES + 1), dict(L=MAX_LABELS + 1), dict(B=MAX_BATCH + 1), dict(B=MAX_BATCH, T=32769), dict(B=2, T=2 ** 30)):
        assert _loss(lib, **kw) == WN_ERR_UNSUPPORTED, kw
    for name in ("x", "labels", "label_len", "nll", "ws"):
        assert _loss(lib, **{name: None}) == WN_ERR_NULL, name
    need = lib.wn_ctc_workspace_bytes(2, 5, 10, 4)
    assert need == _bytes(2, 10, 4)
    assert _loss(lib, ws_bytes=need - 1) == WN_ERR_WORKSPACE
    assert _loss(lib, ws_bytes=0) == WN_ERR_WORKSPACE
    for off in (1, 2, 4, 7):
        assert _loss(lib, ws=ctypes.c_void_p((1 << 20) + off)) == WN_ERR_WORKSPACE, off      # not 8-byte aligned


def test_the_order_of_the_checks(lib):
    """shape, then unsupported, then NULL, then workspace"""
    assert _loss(lib, B=0, C=65, x=None, ws_bytes=0) == WN_ERR_BAD_SHAPE
    assert _loss(lib, blank=7, L=2048, x=None, ws_bytes=0) == WN_ERR_BAD_SHAPE
    assert _loss(lib, C=65, x=None, ws_bytes=0) == WN_ERR_UNSUPPORTED
    assert _loss(lib, x=None, ws_bytes=0) == WN_ERR_NULL
    assert _loss(lib, ws=None, ws_bytes=0) == WN_ERR_NULL
    assert _loss(lib, ws=ctypes.c_void_p((1 << 20) + 4), ws_bytes=0) == WN_ERR_WORKSPACE


def test_the_limits_themselves_are_accepted(lib):
    """at C = 64, L = 2047, B = 65535 every check up to the workspace's passes: one byte short is the first complaint"""
    for kw in (dict(C=MAX_CLASSES, blank=63), dict(L=MAX_LABELS), dict(B=MAX_BATCH), dict(B=MAX_BATCH, T=32768, L=1),
               dict(B=1, C=MAX_CLASSES, T=2304, L=MAX_LABELS)):
        shape = dict(B=2, C=5, T=10, L=4)
        shape.update({k: v for k, v in kw.items() if k in shape})
        need = lib.wn_ctc_workspace_bytes(shape["B"], shape["C"], shape["T"], shape["L"])
        assert need == _bytes(shape["B"], shape["T"], shape["L"]) > 0, kw
        assert _loss(lib, ws_bytes=need - 1, **kw) == WN_ERR_WORKSPACE, kw


def test_the_documented_limits_match():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        text = f.read()
    line = next(l for l in text.splitlines() if "limits (checked, WN_ERR_UNSUPPORTED otherwise)" in l)
    m = re.search(r"C <= (\d+) classes, Lmax <= (\d+) labels per utterance, B <= (\d+), B\*T < 2\^(\d+)", line)
    assert m, line
    assert tuple(int(v) for v in m.groups()) == (MAX_CLASSES, MAX_LABELS, MAX_BATCH, 31)
