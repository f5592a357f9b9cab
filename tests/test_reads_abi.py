"""CPU: the C ABI of the ragged read generator (csrc/wn_reads.hip): exported symbols, the ctypes table against the header, the
workspace formula, and the shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls
below touches a device."""
import ctypes
import re

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, check_row, header_text

FIXED, UNIFORM, GAMMA = 0, 1, 2
NAMES = ("wn_reads_workspace_bytes", "wn_reads_plan", "wn_reads_signal")


@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_reads_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.wn_version() == 300                                   # additive entry points


def test_signature_table_matches_the_header():
    for name in NAMES:
        check_row(name, opaque=True)
    assert re.search(r"WN_DWELL_FIXED = 0, WN_DWELL_UNIFORM = 1, WN_DWELL_GAMMA = 2", header_text())


def test_workspace_bytes(lib):
    for B, n in [(1, 1), (1, 10), (32, 701), (16, 2700), (3, 8), (3, 9), (65535, 30), (2, 65536)]:
        got = lib.wn_reads_workspace_bytes(B, n)
        assert got == B * ((n + 7) // 8 * 8) * 2, (B, n)             # one 16-bit 5-mer index per k-mer, rows of a multiple of 8
        assert got % 16 == 0 and got >= B * (n - 4) * 2
    for B, n in [(0, 10), (-1, 10), (4, 0), (4, -2), (65536, 10), (4, 65537)]:
        assert lib.wn_reads_workspace_bytes(B, n) == 0, (B, n)


def _plan(lib, B=2, lo=20, hi=30, window=2, model=UNIFORM, p=(6.0, 2.0, 0.0), max_dwell=7, lengths_in=None, bases_in=None, dwell_in=None,
          base_lengths=FAKE, bases=FAKE, dwell=FAKE, starts=FAKE, signal_lengths=FAKE, ws=FAKE, ws_bytes=1 << 40):
    return lib.wn_reads_plan(1, B, lo, hi, window, model, p[0], p[1], p[2], max_dwell, lengths_in, bases_in, dwell_in, base_lengths,
                             bases, dwell, starts, signal_lengths, ws, ws_bytes, None, None, None)


def test_reads_plan_rejects_on_the_host(lib):
    # shapes and parameters
    for kw in (dict(B=0), dict(B=-2), dict(hi=0), dict(max_dwell=0), dict(window=1), dict(window=-2), dict(window=3),
               dict(lo=8), dict(lo=4, window=0), dict(lo=30), dict(lo=31), dict(model=3), dict(model=-1),
               dict(model=FIXED, p=(0.0, 0.0, 0.0)), dict(model=UNIFORM, p=(0.0, 2.0, 0.0)), dict(model=UNIFORM, p=(1.0, 0.0, 0.0)),
               dict(model=UNIFORM, p=(6.0, -1.0, 0.0)), dict(model=UNIFORM, p=(6.0, 0.0, 0.0)), dict(model=GAMMA, p=(0.0, 1.0, 1.0)),
               dict(model=GAMMA, p=(1.0, 0.0, 1.0)), dict(model=GAMMA, p=(1.0, 1.0, -4.0)), dict(model=GAMMA, p=(float("nan"), 1.0, 1.0)),
               dict(model=GAMMA, p=(1.0, float("inf"), 1.0))):
        assert _plan(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    # every limit: WN_ERR_UNSUPPORTED
    assert _plan(lib, B=65536) == WN_ERR_UNSUPPORTED
    assert _plan(lib, hi=65537) == WN_ERR_UNSUPPORTED
    assert _plan(lib, hi=1005, max_dwell=2147484) == WN_ERR_UNSUPPORTED         # 1000 * 2147484 = 2^31 + 352
    # the accepted side of each edge goes on to the pointer checks
    assert _plan(lib, B=65535, base_lengths=None) == WN_ERR_NULL
    assert _plan(lib, hi=65536, base_lengths=None) == WN_ERR_NULL
    assert _plan(lib, hi=1005, max_dwell=2147483, base_lengths=None) == WN_ERR_NULL      # 1000 * 2147483 = 2^31 - 648
    assert _plan(lib, lo=9, base_lengths=None) == WN_ERR_NULL
    assert _plan(lib, lo=5, window=0, base_lengths=None) == WN_ERR_NULL
    assert _plan(lib, lo=29, base_lengths=None) == WN_ERR_NULL
    assert _plan(lib, model=UNIFORM, p=(1.0, 1.0, 0.0), base_lengths=None) == WN_ERR_NULL             # [1, 2)
    assert _plan(lib, model=GAMMA, p=(0.5, 587.0, 4000.0), base_lengths=None) == WN_ERR_NULL
    # required pointers; the three *_in, bad and clamped are optional (they are NULL in every call here)
    for name in ("base_lengths", "bases", "dwell", "starts", "signal_lengths", "ws"):
        assert _plan(lib, **{name: None}) == WN_ERR_NULL, name
    need = lib.wn_reads_workspace_bytes(2, 30)
    assert need == 2 * 32 * 2
    assert _plan(lib, ws_bytes=need - 1) == WN_ERR_WORKSPACE
    assert _plan(lib, ws_bytes=0) == WN_ERR_WORKSPACE
    assert _plan(lib, ws=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE             # not 16-byte aligned
    # the order of the checks: shape, then unsupported, then NULL, then workspace
    assert _plan(lib, B=0, hi=65537, bases=None) == WN_ERR_BAD_SHAPE
    assert _plan(lib, window=1, B=65536, bases=None) == WN_ERR_BAD_SHAPE
    assert _plan(lib, B=65536, bases=None, ws_bytes=0) == WN_ERR_UNSUPPORTED
    assert _plan(lib, bases=None, ws_bytes=0) == WN_ERR_NULL


def test_limit_edge_of_the_signal_length(lib):
    # (max_bases - 5) * max_dwell < 2^31 exactly: 65531 * 32771 = 2147516401 >= 2^31 > 65531 * 32770 = 2147450870
    assert 65531 * 32770 < 2 ** 31 <= 65531 * 32771
    assert _plan(lib, hi=65536, max_dwell=32771) == WN_ERR_UNSUPPORTED
    assert _plan(lib, hi=65536, max_dwell=32770, base_lengths=None) == WN_ERR_NULL


def _signal(lib, B=2, hi=30, window=2, ld=100, base_lengths=FAKE, starts=FAKE, signal_lengths=FAKE, ws=FAKE, ws_bytes=1 << 40, means=FAKE,
            stdvs=FAKE, signal=FAKE):
    return lib.wn_reads_signal(base_lengths, starts, signal_lengths, ws, ws_bytes, B, hi, window, ld, means, stdvs, 1, None, signal,
                               None, None, None, None)


def test_reads_signal_rejects_on_the_host(lib):
    for kw in (dict(B=0), dict(hi=0), dict(ld=0), dict(ld=-5), dict(window=1), dict(window=4)):
        assert _signal(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    assert _signal(lib, B=65536) == WN_ERR_UNSUPPORTED
    assert _signal(lib, hi=65537) == WN_ERR_UNSUPPORTED
    assert _signal(lib, ld=2 ** 31 - 256) == WN_ERR_UNSUPPORTED
    assert _signal(lib, ld=2 ** 31 - 257, signal=None) == WN_ERR_NULL
    for name in ("base_lengths", "starts", "signal_lengths", "ws", "means", "stdvs", "signal"):
        assert _signal(lib, **{name: None}) == WN_ERR_NULL, name
    need = lib.wn_reads_workspace_bytes(2, 30)
    assert _signal(lib, ws_bytes=need - 1) == WN_ERR_WORKSPACE
    assert _signal(lib, ws=ctypes.c_void_p((1 << 20) + 4)) == WN_ERR_WORKSPACE
    assert _signal(lib, ld=0, B=65536, signal=None) == WN_ERR_BAD_SHAPE
    assert _signal(lib, B=65536, signal=None, ws_bytes=0) == WN_ERR_UNSUPPORTED
    assert _signal(lib, signal=None, ws_bytes=0) == WN_ERR_NULL
