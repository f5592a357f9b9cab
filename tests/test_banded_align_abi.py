"""CPU: the C ABI of banded alignment (csrc/wn_bandalign.hip): exported symbols, the ctypes table against the header, the workspace
formula, the shape / limit / pointer checks in their documented order, which run on the host before any HIP call -- none of the
calls below touches a device -- and the refusals of the Python surface that need no device."""
import ctypes

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry, host_alignment
from tests.abi_util import lib  # noqa: F401

BAND = Entry("wn_banded_align", dict(ref=FAKE, ref_stride=lambda a: a["max_ref_len"], ref_lengths=FAKE, query=FAKE,
                                     query_stride=lambda a: a["max_query_len"], query_lengths=FAKE, diag_lo=FAKE, diag_hi=FAKE, batch=2,
                                     max_ref_len=10, max_query_len=12, max_band=5, match=10, mismatch=-8, gap_open=20, gap_extend=1,
                                     end_gaps_free=1, score=FAKE, stats=FAKE, ops=FAKE, ops_len=FAKE, status=FAKE, edge_hits=FAKE,
                                     workspace=FAKE, workspace_bytes=1 << 50, bad=None, stream=None))
SIZE = Entry("wn_banded_align_workspace_bytes", dict(batch=2, max_ref_len=10, max_query_len=12, max_band=5))


def test_banded_align_symbols_are_exported(lib):
    BAND.check_exported(lib)
    SIZE.check_exported(lib)


def test_signature_table_matches_the_header():
    BAND.check_declared()                                            # 27 arguments
    SIZE.check_declared()                                            # 4


def _want_bytes(B, N, M, band):
    T = (band + 7) // 8                                              # threads that own a diagonal: 8 diagonals each
    bp = B * (N + M + 1) * T * 2                                     # one 16-bit word per thread and step, N + M + 1 steps
    return (bp + 15) // 16 * 16 + B * ((N + M + 15) // 16 * 16)      # and the path's ops back to front, one byte each


def test_workspace_bytes(lib):
    for B, N, M, band in [(1, 1, 1, 1), (32, 400, 410, 64), (4096, 1200, 1200, 128), (1, 8192, 8192, 256), (1, 65535, 65535, 2048),
                          (3, 77, 9, 7), (3, 77, 9, 8), (3, 77, 9, 9), (65535, 1, 1, 1), (2, 65535, 300, 513)]:
        n = lib.wn_banded_align_workspace_bytes(B, N, M, band)
        assert n == _want_bytes(B, N, M, band), (B, N, M, band)
        assert n % 16 == 0
        assert n >= B * ((N + M + 1) * (band // 2) // 2 + N + M)     # 4 bits per in-band cell of a step (half the width), a byte per op
        assert n <= B * ((N + M + 1) * ((band + 7) // 8 * 8) // 4 + N + M + 15) + 15     # and no more, but for the padding
    # one 8192 x 8192 pair at width 256: about 1 / 34 of the full matrix's backpointers
    assert lib.wn_banded_align_workspace_bytes(1, 8192, 8192, 256) * 16 <= lib.wn_pair_align_workspace_bytes(1, 8192, 8192)
    assert lib.wn_banded_align_workspace_bytes(4096, 1200, 1200, 128) < 1 << 30
    for B, N, M, band in [(0, 10, 10, 5), (8, 0, 10, 5), (8, 10, 0, 5), (8, 10, 10, 0), (-1, 10, 10, 5), (8, -3, 10, 5), (8, 10, -1, 5),
                          (8, 10, 10, -2), (65536, 10, 10, 5), (8, 65536, 10, 5), (8, 10, 65536, 5), (8, 10, 10, 2049)]:
        assert lib.wn_banded_align_workspace_bytes(B, N, M, band) == 0, (B, N, M, band)


def test_banded_align_rejects_on_the_host(lib):
    BAND.rejects(lib, "ref",
                 shape=(dict(batch=0), dict(batch=-1), dict(max_ref_len=0), dict(max_query_len=0), dict(max_query_len=-4), dict(max_band=0),
                        dict(max_band=-1)),
                 # every limit: WN_ERR_UNSUPPORTED, nothing launched
                 unsupported=(dict(max_band=2049), dict(max_ref_len=65536), dict(max_query_len=65536), dict(batch=65536),
                              dict(gap_open=1025), dict(gap_extend=21), dict(gap_extend=-1), dict(gap_open=-1, gap_extend=-2),
                              dict(match=1025), dict(match=-1025), dict(mismatch=1025), dict(mismatch=-1025)),
                 # the other side of each
                 accepted=(dict(max_band=1), dict(max_band=2048), dict(max_ref_len=65535), dict(max_query_len=65535), dict(max_query_len=8193),
                           dict(batch=1), dict(batch=65535), dict(gap_open=1024), dict(gap_extend=20), dict(gap_extend=0),
                           dict(match=1024), dict(match=-1024), dict(mismatch=1024), dict(mismatch=-1024), dict(edge_hits=None),
                           dict(stats=None), dict(bad=FAKE)),
                 # required pointers; ops and ops_len come together; stats or ops need the workspace
                 required=("ref", "ref_lengths", "query", "query_lengths", "diag_lo", "diag_hi", "score", "status", "ops", "ops_len",
                           "workspace"))
    assert BAND(lib, stats=None, workspace=None) == WN_ERR_NULL                          # ops still want it
    assert BAND(lib, stats=None, ops=None, ops_len=None, workspace=None) == WN_ERR_NULL  # score only: edge_hits must be NULL
    need = SIZE(lib)
    assert need > 0
    assert BAND(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert BAND(lib, workspace_bytes=0) == WN_ERR_WORKSPACE
    assert BAND(lib, ops=None, ops_len=None, workspace_bytes=need - 1) == WN_ERR_WORKSPACE             # stats alone need it too
    assert BAND(lib, workspace=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE                     # not 16-byte aligned
    # the documented order: shape; max_band, max_ref_len, max_query_len, batch, the costs; NULL; the workspace
    assert BAND(lib, batch=0, max_band=2049, ref=None) == WN_ERR_BAD_SHAPE
    assert BAND(lib, max_band=2049, ref=None, workspace_bytes=0) == WN_ERR_UNSUPPORTED
    assert BAND(lib, gap_extend=21, ref=None) == WN_ERR_UNSUPPORTED
    assert BAND(lib, ref=None, workspace_bytes=0) == WN_ERR_NULL


def test_python_refusals_without_a_device():
    import torch
    import wavenet_speech_amd as W
    rows, n = torch.ones(2, 5, dtype=torch.int32), torch.tensor([5, 5])
    with pytest.raises(RuntimeError):                                # host rows: there is no CPU fallback
        W.banded_align(rows, n, rows, n, [0, 0], [1, 1], 2)
    with pytest.raises(ValueError, match="multiple of 0.5"):                   # costs are checked first, as in pairwise_align
        W.banded_align(rows, n, rows, n, [0, 0], [1, 1], 2, gap_extend=0.3)
    with pytest.raises(RuntimeError):
        W.band_from_ops(host_alignment())
    with pytest.raises(ValueError):
        W.band_from_ops(None)
    assert W.BandedAlignment._fields == ("alignment", "status", "edge_hits", "diag_lo", "diag_hi")
