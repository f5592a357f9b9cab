"""CPU: the C ABI of pairwise alignment (csrc/wn_pairalign.hip): exported symbols, the ctypes table against the header, the
workspace formula, and the shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls
below touches a device."""
import ctypes

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

PAIR = Entry("wn_pair_align", dict(ref=FAKE, ref_stride=lambda a: a["max_ref_len"], ref_lengths=FAKE, query=FAKE,
                                   query_stride=lambda a: a["max_query_len"], query_lengths=FAKE, batch=2, max_ref_len=10, max_query_len=12,
                                   match=10, mismatch=-8, gap_open=20, gap_extend=1, end_gaps_free=1, score=FAKE, stats=FAKE, ops=FAKE,
                                   ops_len=FAKE, workspace=FAKE, workspace_bytes=1 << 40, bad=None, stream=None))
SIZE = Entry("wn_pair_align_workspace_bytes", dict(batch=2, max_ref_len=10, max_query_len=12))


def test_pair_align_symbols_are_exported(lib):
    PAIR.check_exported(lib)
    SIZE.check_exported(lib)


def test_signature_table_matches_the_header():
    PAIR.check_declared()                                            # 22 arguments
    SIZE.check_declared()                                            # 3


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


def test_pair_align_rejects_on_the_host(lib):
    PAIR.rejects(lib, "ref",
                 shape=(dict(batch=0), dict(max_ref_len=0), dict(max_query_len=0), dict(max_query_len=-4)),         # non-positive shapes
                 # every limit: WN_ERR_UNSUPPORTED, nothing launched
                 unsupported=(dict(max_query_len=8193), dict(max_ref_len=65536), dict(batch=65536),
                              dict(gap_open=1025),                   # gap_open > 1024
                              dict(gap_extend=21),                   # gap_extend > gap_open
                              dict(gap_extend=-1),                   # gap_extend < 0
                              dict(gap_open=-1, gap_extend=-2), dict(match=1025), dict(match=-1025), dict(mismatch=1025), dict(mismatch=-1025)),
                 # required pointers; ops and ops_len come together; stats or ops need the workspace
                 required=("ref", "ref_lengths", "query", "query_lengths", "score", "ops", "ops_len", "workspace"))
    assert PAIR(lib, stats=None, workspace=None) == WN_ERR_NULL                          # ops still want it
    need = SIZE(lib)
    assert need > 0
    assert PAIR(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert PAIR(lib, workspace_bytes=0) == WN_ERR_WORKSPACE
    assert PAIR(lib, ops=None, ops_len=None, workspace_bytes=need - 1) == WN_ERR_WORKSPACE             # stats alone need it too
    assert PAIR(lib, workspace=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE                     # not 16-byte aligned
    # the order of the checks: shape, then unsupported, then NULL, then workspace
    assert PAIR(lib, batch=0, max_query_len=8193, ref=None) == WN_ERR_BAD_SHAPE
    assert PAIR(lib, max_query_len=8193, ref=None, workspace_bytes=0) == WN_ERR_UNSUPPORTED
    assert PAIR(lib, gap_extend=21, ref=None) == WN_ERR_UNSUPPORTED
    assert PAIR(lib, ref=None, workspace_bytes=0) == WN_ERR_NULL
