"""CPU: the C ABI of pairwise alignment (csrc/wn_pairalign.hip): exported symbols, the ctypes table against the header, the
workspace formula, and the shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls
below touches a device."""
import ctypes

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, check_row



@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_pair_align_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for name in ("wn_pair_align_workspace_bytes", "wn_pair_align"):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.wn_version() == 300                                   # an additive entry point


def test_signature_table_matches_the_header():
    for name in ("wn_pair_align_workspace_bytes", "wn_pair_align"):
        check_row(name, opaque=True)


def _want_bytes(B, N, M):
    W = (M + 7) // 8                                                 # threads that own a column: 8 columns each
    bp = B * (N + W - 1) * W * 4                                     # one dword per thread and step, N + W - 1 steps
    return (bp + 15) // 16 * 16 + B * ((N + M + 15) // 16 * 16)      # and the path's ops back to front, one byte each


def test_workspace_bytes(lib):
    for B, N, M in [(1, 1, 1), (8, 400, 400), (32, 410, 390), (1, 8192, 8192), (1, 64, 8192), (1, 4096, 64), (3, 77, 9), (2, 65535, 8),
                    (65535, 1, 1), (5, 100, 513)]:
        n = lib.wn_pair_align_workspace_bytes(B, N, M)
        assert n == _want_bytes(B, N, M), (B, N, M)
        assert n % 16 == 0
        assert n >= B * (N * M // 2 + N + M)                         # 4 bits per cell, one byte per op
    assert lib.wn_pair_align_workspace_bytes(1, 8192, 8192) < 40 << 20
    for B, N, M in [(0, 10, 10), (8, 0, 10), (8, 10, 0), (-1, 10, 10), (8, -3, 10), (8, 10, -1), (65536, 10, 10), (8, 65536, 10),
                    (8, 10, 8193)]:
        assert lib.wn_pair_align_workspace_bytes(B, N, M) == 0, (B, N, M)


def _call(lib, B=2, N=10, M=12, costs=(10, -8, 20, 1), free=1, ref=FAKE, ref_len=FAKE, query=FAKE, query_len=FAKE, score=FAKE,
          stats=FAKE, ops=FAKE, ops_len=FAKE, ws=FAKE, ws_bytes=1 << 40):
    return lib.wn_pair_align(ref, N, ref_len, query, M, query_len, B, N, M, costs[0], costs[1], costs[2], costs[3], free, score,
                             stats, ops, ops_len, ws, ws_bytes, None, None)


def test_pair_align_rejects_on_the_host(lib):
    # every limit: WN_ERR_UNSUPPORTED, nothing launched
    assert _call(lib, M=8193) == WN_ERR_UNSUPPORTED
    assert _call(lib, N=65536) == WN_ERR_UNSUPPORTED
    assert _call(lib, B=65536) == WN_ERR_UNSUPPORTED
    assert _call(lib, costs=(10, -8, 1025, 1)) == WN_ERR_UNSUPPORTED         # gap_open > 1024
    assert _call(lib, costs=(10, -8, 20, 21)) == WN_ERR_UNSUPPORTED          # gap_extend > gap_open
    assert _call(lib, costs=(10, -8, 20, -1)) == WN_ERR_UNSUPPORTED          # gap_extend < 0
    assert _call(lib, costs=(10, -8, -1, -2)) == WN_ERR_UNSUPPORTED
    assert _call(lib, costs=(1025, -8, 20, 1)) == WN_ERR_UNSUPPORTED
    assert _call(lib, costs=(-1025, -8, 20, 1)) == WN_ERR_UNSUPPORTED
    assert _call(lib, costs=(10, 1025, 20, 1)) == WN_ERR_UNSUPPORTED
    assert _call(lib, costs=(10, -1025, 20, 1)) == WN_ERR_UNSUPPORTED
    # non-positive shapes
    assert _call(lib, B=0) == WN_ERR_BAD_SHAPE
    assert _call(lib, N=0) == WN_ERR_BAD_SHAPE
    assert _call(lib, M=0) == WN_ERR_BAD_SHAPE
    assert _call(lib, M=-4) == WN_ERR_BAD_SHAPE
    # required pointers; ops and ops_len come together; stats or ops need the workspace
    for name in ("ref", "ref_len", "query", "query_len", "score", "ops", "ops_len", "ws"):
        assert _call(lib, **{name: None}) == WN_ERR_NULL, name
    assert _call(lib, stats=None, ws=None) == WN_ERR_NULL                    # ops still want it
    need = lib.wn_pair_align_workspace_bytes(2, 10, 12)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == WN_ERR_WORKSPACE
    assert _call(lib, ws_bytes=0) == WN_ERR_WORKSPACE
    assert _call(lib, ops=None, ops_len=None, ws_bytes=need - 1) == WN_ERR_WORKSPACE     # stats alone need it too
    assert _call(lib, ws=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE             # not 16-byte aligned
    # the order of the checks: shape, then unsupported, then NULL, then workspace
    assert _call(lib, B=0, M=8193, ref=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, M=8193, ref=None, ws_bytes=0) == WN_ERR_UNSUPPORTED
    assert _call(lib, costs=(10, -8, 20, 21), ref=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, ref=None, ws_bytes=0) == WN_ERR_NULL
