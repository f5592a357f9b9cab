"""CPU: the C ABI of the realignment step (csrc/wn_realign.hip): the exported symbols, the ctypes rows against the header argument by
argument, and every host-side rejection on both sides of every limit and in its documented order (shape, unsupported, NULL,
workspace), with fake pointers: every call below returns before anything would be launched.  And the host side of the Python
surface: the refusals, "no CPU fallback", and haplotype_calls -- torch ops on any device -- against the reference, S == 0 and the
one haplotype of a ConsensusCalls included."""
import ctypes

import numpy as np
import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry, host_alignment
from tests.abi_util import hand_made_genotypes, lib  # noqa: F401

WINDOWS = Entry("wn_haplotype_windows", dict(call=FAKE, ins_len=FAKE, ins_bases=FAKE, reference=FAKE, lo=FAKE, ref_lengths=FAKE, strand=FAKE,
                                             haplotypes=2, batch=3, reference_len=5000, max_ins=4, max_hap_ops=900, labels=FAKE, lengths=FAKE,
                                             ops=FAKE, ops_len=FAKE, used=FAKE, bad=None, stream=None))
LIFT = Entry("wn_lift_ops", dict(a_ops=FAKE, a_hap_stride=3 * 1300, a_stride=1300, a_ops_len=FAKE, a_max_ops=1300, hap_ops=FAKE, hap_hap_stride=3 * 900,
                                 hap_stride=900, hap_ops_len=FAKE, hap_lengths=FAKE, max_hap_ops=900, max_hap_len=900, used=FAKE, pick=FAKE, ref=FAKE,
                                 ref_stride=500, ref_lengths=FAKE, query=FAKE, query_stride=400, query_lengths=FAKE, haplotypes=2, batch=3,
                                 max_ref_len=500, max_query_len=400, max_ops=900, match=10, mismatch=-8, gap_open=20, gap_extend=1, end_gaps_free=1,
                                 ops=FAKE, ops_stride=900, ops_len=FAKE, score=FAKE, stats=FAKE, workspace=FAKE,
                                 workspace_bytes=lambda a: 12 * a["batch"] * (a["max_hap_len"] + 1), bad=None, stream=None))


def test_symbols_are_exported(lib):
    for entry in (WINDOWS, LIFT):
        entry.check_exported(lib)
    from wavenet_speech_amd import _lib
    assert "wn_lift_ops_workspace_bytes" in _lib.SIGNATURES and hasattr(lib, "wn_lift_ops_workspace_bytes")


def test_signature_rows_match_the_header():
    from tests.abi_util import check_row
    WINDOWS.check_declared()                                         # 19 arguments
    LIFT.check_declared()                                            # 39
    check_row("wn_lift_ops_workspace_bytes", count=2)


def test_haplotype_windows_rejects_on_the_host_in_order(lib):
    WINDOWS.rejects(lib, "call",
                    shape=(dict(haplotypes=0), dict(haplotypes=-1), dict(batch=0), dict(batch=-1), dict(reference_len=0), dict(max_ins=-1),
                           dict(max_hap_ops=0)),
                    unsupported=(dict(haplotypes=3), dict(batch=65536), dict(reference_len=2 ** 26 + 1), dict(max_ins=9), dict(max_hap_ops=65536)),
                    accepted=(dict(haplotypes=1), dict(haplotypes=2), dict(batch=1), dict(batch=65535), dict(reference_len=1), dict(reference_len=2 ** 26),
                              dict(max_ins=0, ins_bases=None), dict(max_ins=8), dict(max_hap_ops=1), dict(max_hap_ops=65535), dict(bad=FAKE)),
                    required=("call", "ins_len", "ins_bases", "reference", "lo", "ref_lengths", "strand", "labels", "lengths", "ops", "ops_len", "used"))
    assert WINDOWS(lib, batch=0, haplotypes=3, call=None) == WN_ERR_BAD_SHAPE                   # the order: shape, unsupported, NULL
    assert WINDOWS(lib, max_hap_ops=0, reference_len=2 ** 26 + 1) == WN_ERR_BAD_SHAPE
    assert WINDOWS(lib, max_ins=9, call=None) == WN_ERR_UNSUPPORTED


def test_lift_ops_rejects_on_the_host_in_order(lib):
    ints = ("haplotypes", "batch", "max_hap_len", "a_max_ops", "max_hap_ops", "max_ref_len", "max_query_len", "max_ops")
    strides = ("a_hap_stride", "a_stride", "hap_hap_stride", "hap_stride", "ref_stride", "query_stride", "ops_stride")
    LIFT.rejects(lib, "a_ops",
                 shape=tuple({n: 0} for n in ints) + (dict(batch=-1),) + tuple({n: -1} for n in strides) + (dict(end_gaps_free=2), dict(end_gaps_free=-1)),
                 unsupported=(dict(haplotypes=3), dict(batch=65536), dict(max_hap_len=65536), dict(max_hap_ops=65536), dict(max_ref_len=65536),
                              dict(max_query_len=8193), dict(a_max_ops=65535 + 8192 + 1), dict(max_ops=65535 + 8192 + 1), dict(gap_open=1025),
                              dict(gap_extend=21), dict(gap_extend=-1), dict(match=1025), dict(mismatch=-1025)),
                 accepted=(dict(haplotypes=1), dict(batch=1), dict(batch=65535), dict(max_hap_len=1), dict(max_hap_len=65535), dict(max_hap_ops=1),
                           dict(max_hap_ops=65535), dict(max_ref_len=1), dict(max_ref_len=65535), dict(max_query_len=1), dict(max_query_len=8192),
                           dict(a_max_ops=1), dict(a_max_ops=65535 + 8192), dict(max_ops=1), dict(max_ops=65535 + 8192), dict(a_hap_stride=0),
                           dict(end_gaps_free=0), dict(gap_open=1024, gap_extend=1024), dict(match=-1024, mismatch=1024), dict(bad=FAKE)),
                 required=("a_ops", "a_ops_len", "hap_ops", "hap_ops_len", "hap_lengths", "used", "pick", "ref", "ref_lengths", "query", "query_lengths",
                           "ops", "ops_len", "score", "stats", "workspace"))
    assert LIFT(lib, batch=0, haplotypes=3, a_ops=None) == WN_ERR_BAD_SHAPE                     # the order: shape, unsupported, NULL, workspace
    assert LIFT(lib, ops_stride=-1, max_hap_len=65536) == WN_ERR_BAD_SHAPE
    assert LIFT(lib, max_query_len=8193, a_ops=None) == WN_ERR_UNSUPPORTED
    assert LIFT(lib, gap_open=1025, a_ops=None) == WN_ERR_UNSUPPORTED
    assert LIFT(lib, a_ops=None, workspace_bytes=0) == WN_ERR_NULL
    need = 12 * 3 * 901
    assert lib.wn_lift_ops_workspace_bytes(3, 900) == need
    assert LIFT(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert LIFT(lib, workspace=ctypes.c_void_p((1 << 20) + 2)) == WN_ERR_WORKSPACE
    for batch, width in ((0, 900), (65536, 900), (3, 0), (3, 65536)):
        assert lib.wn_lift_ops_workspace_bytes(batch, width) == 0
    assert lib.wn_lift_ops_workspace_bytes(65535, 65535) == 12 * 65535 * 65536


def _host_calls(H=2, R=40, max_ins=2):
    import wavenet_speech_amd as W
    return W.HaplotypeCalls(torch.ones(H, R, dtype=torch.uint8), torch.zeros(H, R, dtype=torch.uint8), torch.zeros(H, R, max_ins, dtype=torch.uint8))


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    hcalls = _host_calls()
    reads = dict(lo=[0, 5], ref_lengths=[30, 30], strand=[0, 1])
    with pytest.raises(ValueError, match="wavenet_speech_amd.haplotype_windows: hcalls must be HaplotypeCalls"):
        W.haplotype_windows(hcalls.call, torch.ones(40), **reads)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.haplotype_windows: hcalls.call must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.haplotype_windows(hcalls, torch.ones(40, dtype=torch.int32), **reads)
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.realign: hcalls.call must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.realign(torch.ones(2, 30, dtype=torch.int32), [30, 30], torch.ones(2, 30, dtype=torch.int32), [30, 30], [0, 5], [0, 1], hcalls,
                  torch.ones(40, dtype=torch.int32))
    query, n = torch.ones(2, 30, dtype=torch.int32), [30, 30]
    windows = W.HaplotypeWindows(None, torch.zeros(2, 2, dtype=torch.int32), torch.ones(2, 2, 30, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32),
                                 torch.ones(2, dtype=torch.int8))
    args = dict(alignments=[host_alignment(), host_alignment()], windows=windows, pick=[0, 1], ref=query, ref_lengths=n, query=query, query_lengths=n)
    with pytest.raises(ValueError, match="wavenet_speech_amd.lift_alignment: alignment must be a PairwiseAlignment with ops"):
        W.lift_alignment(**dict(args, alignments=[W.PairwiseAlignment(None, None, None, None, None, None, None)]))
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.lift_alignment: alignment.ops must be a GPU tensor \\(there is no CPU fallback\\)"):
        W.lift_alignment(**args)
    with pytest.raises(ValueError, match="wavenet_speech_amd.lift_alignment: alignments must be one PairwiseAlignment per haplotype"):
        W.lift_alignment(**dict(args, alignments=[host_alignment()] * 3))
    with pytest.raises(ValueError, match="wavenet_speech_amd.lift_alignment: gap_extend must be a multiple of 0.5"):
        W.lift_alignment(**dict(args, gap_extend=0.3))
    with pytest.raises(ValueError, match="wavenet_speech_amd.lift_alignment: need 0 <= gap_extend <= gap_open"):
        W.lift_alignment(**dict(args, gap_open=1, gap_extend=2))
    with pytest.raises(ValueError, match="wavenet_speech_amd.haplotype_calls: genotypes must be Genotypes or ConsensusCalls"):
        W.haplotype_calls(torch.zeros(4, dtype=torch.uint8))
    ref, g, pile = hand_made_genotypes()
    with pytest.raises(ValueError, match="wavenet_speech_amd.haplotype_calls: Genotypes need sites, a PhaseSites, and phasing, a Phasing"):
        W.haplotype_calls(g)
    calls = W.ConsensusCalls(torch.ones(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), torch.zeros(8, 2, dtype=torch.uint8), None, None, None, None)
    with pytest.raises(ValueError, match="wavenet_speech_amd.haplotype_calls: a ConsensusCalls is one haplotype"):
        W.haplotype_calls(calls, sites=1)
    with pytest.raises(ValueError, match="wavenet_speech_amd.haplotype_calls: calls.ins_len must be a uint8 tensor"):
        W.haplotype_calls(calls._replace(ins_len=torch.zeros(8, dtype=torch.int32)))
    with pytest.raises(ValueError, match="wavenet_speech_amd.haplotype_calls: calls must hold call \\(R,\\)"):
        W.haplotype_calls(calls._replace(ins_len=torch.zeros(7, dtype=torch.uint8)))


def _hand_phased():
    """the hand-made genotypes with the sites and the chain of tests/phase_cases.py as tensors, and the same for the reference"""
    import wavenet_speech_amd as W
    from tests import phase_ref as H
    from tests.phase_cases import HAND_CHAIN, hand_calls
    ref, g, pile = hand_made_genotypes()
    _, calls, _ = hand_calls()
    host_sites = H.sites_ref(calls.flags, calls.alleles)
    site_of = torch.tensor(host_sites.site_of, dtype=torch.int32)
    sites = W.PhaseSites(torch.tensor(host_sites.pos, dtype=torch.int32), g.alleles[host_sites.pos], site_of)
    dtypes = (torch.int32, torch.uint8, torch.int32, torch.int32, torch.uint8, torch.int32, torch.int32)
    return g, sites, W.Phasing(*[torch.tensor(v, dtype=d) for v, d in zip(HAND_CHAIN, dtypes)]), calls, host_sites, HAND_CHAIN


def _same(got, want):
    return all(t.dtype == torch.uint8 and t.is_contiguous() and np.array_equal(t.numpy(), w) for t, w in zip(got, want))


def test_haplotype_calls_agree_with_the_reference_with_no_site_and_with_one_haplotype():
    import wavenet_speech_amd as W
    from tests import pileup_ref as P
    from tests import realign_ref as RR
    g, sites, phasing, calls, host_sites, chain = _hand_phased()
    got = W.haplotype_calls(g, sites, phasing)
    assert tuple(got.call.shape) == (2, 8) and tuple(got.ins_bases.shape) == (2, 8, 2)
    assert _same(got, RR.haplotype_calls_ref(calls, host_sites, chain))
    assert got.call.tolist() == [[0, 0, 0, 4, 2, 2, 0, 1], [0, 2, 1, 0, 2, 0, 0, 2]] and not got.ins_len.any()      # the values of tests/test_realign_ref.py
    both = g._replace(ins_copies=torch.tensor([0, 0, 0, 0, 2, 0, 0, 0], dtype=torch.uint8))                          # a homozygous insertion: on both
    assert _same(W.haplotype_calls(both, sites, phasing), RR.haplotype_calls_ref(calls._replace(ins_copies=both.ins_copies.numpy()), host_sites, chain))
    flipped = phasing._replace(parity=1 - phasing.parity)
    swapped = W.haplotype_calls(g, sites, flipped)
    assert torch.equal(swapped.call[0], got.call[1]) and torch.equal(swapped.call[1], got.call[0])
    # S == 0: both haplotypes carry alleles[., 0]
    none = W.PhaseSites(torch.zeros(0, dtype=torch.int32), torch.zeros(0, 2, dtype=torch.uint8), torch.full((8,), -1, dtype=torch.int32))
    empty = W.Phasing(*[torch.zeros(0, dtype=t.dtype) for t in phasing])
    got = W.haplotype_calls(g, none, empty)
    assert torch.equal(got.call[0], g.alleles[:, 0]) and torch.equal(got.call[1], g.alleles[:, 0])
    # H = 1 from a ConsensusCalls
    consensus = P.call_consensus_ref(P.Pile(np.zeros((8, 2, 6), dtype=np.int64), np.zeros((8, 3), dtype=np.int64), np.zeros((8, 2, 4), dtype=np.int64), None, 0),
                                     [1, 2, 3, 4, 1, 2, 3, 4])
    u8 = lambda a: torch.from_numpy(np.asarray(a).astype(np.uint8))  # noqa: E731
    one = W.haplotype_calls(W.ConsensusCalls(u8(consensus.call), u8(consensus.ins_len), u8(consensus.ins_bases), None, None, None, None))
    assert tuple(one.call.shape) == (1, 8) and one.call[0].tolist() == [1, 2, 3, 4, 1, 2, 3, 4] and tuple(one.ins_bases.shape) == (1, 8, 2)
    assert _same(one, RR.haplotype_calls_ref(consensus))
