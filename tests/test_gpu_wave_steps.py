"""GPU: the seams that csrc/wn_wave_dev.h owns -- wave and workgroup scans, wave reductions, the one-lane shift and the neighbour
hand-off of the systolic aligners -- each through the tool that uses it, at the smallest shapes that reach the seam, by exact
equality against the host references of the tools (tests/*_ref.py).  The tools themselves are held by their own files."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import ctc_align_ref as A
from tests import demux_cases as DC
from tests import demux_ref as DR
from tests import event_detect_cases as EC
from tests import kmer_events_cases as KC
from tests import kmer_events_ref as KR
from tests import pairwise_align_ref as PR
from tests import pileup_cases as PC
from tests import pileup_ref as P
from tests import read_stats_ref as SR
from tests import readmap_cases as RC
from tests import readmap_ref as RR
from tests.gpu_calls import assert_consensus, pile_both
from tests.gpu_labels import assert_pick, assert_scores, assert_seeds, check_forced_batch, check_pair_batch, forced_align, kit, kw, pair_align, plan_given
from tests.gpu_signal import assert_detected, assert_kmer_events, detect_events, kmer_events
from tests.gpu_util import DEV, dev
from wavenet_speech_amd import normalise as N

pytestmark = pytest.mark.gpu


# ---- scans ----------------------------------------------------------------------------------------------------------------------

def test_pileup_op_strings_at_the_wave_and_tile_seams():
    """tile_scan (two ballots, wave_offsets) in the walk; block_scan in the call, the scan of the tile totals and the emit"""
    rng = np.random.default_rng(11)
    reads = [PC.read(PC.random_ops(rng, n), rng, quals=False) for n in (63, 64, 65, 255, 256, 257)]
    n, R = len(reads), 300
    for strand in (0, 1):
        got, want = pile_both([r[0] for r in reads], [7 * b for b in range(n)], [r[1] for r in reads], [strand] * n, [r[2] for r in reads], R,
                              max_ins=2)
        assert want.used.tolist() == [1] * n
    ref = rng.integers(1, 5, size=R).astype(np.int32)
    assert_consensus(W.call_consensus(got, dev(ref), min_depth=1, min_fraction=(1, 2)), P.call_consensus_ref(want, ref, 1, 1, 2))
    W.check_device_flags()


@pytest.mark.parametrize("words", [1023, 1024, 1025])
def test_event_ranks_with_boundaries_in_the_first_and_the_last_word(words):
    """block_scan<16> (max, then sum) over one full step of 1024 words, one word less, and one word into a second step"""
    T = 64 * words - 3
    x, _ = EC.steps([50, 70, 50], [20, T - 40, 20])
    case = EC.batch_of([x], EC.kw_of(windows=(3, 0)))
    ref = EC.call_ref(case)
    assert {p >> 6 for p, _ in EC.boundaries(ref, 0) if _ != 3} == {0, words - 1}
    assert_detected(detect_events(case, chunk=None), ref)
    W.check_device_flags()


def test_seed_anchors_with_hits_at_both_ends_of_reads_around_a_tile():
    """block_scan<4> of (minimizer, hits) per tile of 256 positions: 255, 256 and 257 positions, as bases and as k-mer starts"""
    k = 6
    ref = RC.random_bases(np.random.default_rng(12), 700)
    reads = [ref[100:100 + n] for n in (255, 256, 257, 255 + k - 1, 256 + k - 1, 257 + k - 1)]
    got, want = assert_seeds(ref, reads, k, 1, 8, 2048)
    host = RR.index_ref(ref, k, 1)
    for read in reads:
        q = {a[2] for a in RR.anchors_ref(read, host, k, 1, 8, 2048)[0] if a[0] == 0}
        assert 0 in q and len(read) - k in q
    W.check_device_flags()


def test_reads_plan_with_fixed_dwell_1_gives_arange():
    sizes = (255, 256, 257)
    plan = plan_given(None, torch.tensor(sizes) + 4, None, 0)                    # window 0: K = n - 4
    assert int(plan["bad"]) == 0
    for b, K in enumerate(sizes):
        assert torch.equal(plan["starts"][b, :K + 1].cpu().long(), torch.arange(K + 1)) and int(plan["signal_lengths"][b]) == K
    W.check_device_flags()


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_order_statistics_first_and_last_of_257_samples(dtype):
    """wave_scan over the 256 bins of a digit: the first bin that holds anything, and the last"""
    x = np.random.default_rng(13).integers(-30000, 30000, size=(1, 257)).astype(dtype)
    got = N.read_order_statistics(torch.from_numpy(x).to(DEV), torch.tensor([257], dtype=torch.int32, device=DEV),
                                  torch.tensor([[0, 256]], dtype=torch.int32, device=DEV)).cpu().numpy()
    want = [SR.order_statistic(x[0], 257, r) for r in (0, 256)]
    assert got[0].tolist() == [np.float32(v) for v in want] == [np.float32(x.min()), np.float32(x.max())]
    W.check_device_flags()


# ---- reductions -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 63, 64, 65])
@pytest.mark.parametrize("at", ["first", "last"])
def test_demux_with_the_best_and_longest_pattern_at_either_end_of_the_waves(K, at):
    """wave_reduce(max): the longest pattern of a wave in demux_scores, the best key and the runner-up in demux_pick"""
    rng = np.random.default_rng(100 * K + len(at))
    best = DC._rand(rng, 24)
    front = [DC._rand(rng, int(rng.integers(5, 12))) for _ in range(K)]
    front[0 if at == "first" else K - 1] = best
    case = DC._case([DC._rand(rng, 9) + best + DC._rand(rng, 30), DC._rand(rng, 50)], front, [], 48)
    ref = DR.demux_scores_ref(case.labels, case.lengths, case.patterns, case.pattern_lengths, case.n_front, case.window, *case.costs)
    want = DR.demux_pick_ref(ref["score"], ref["start"], ref["end"], case.lengths, case.group, DC.min_scores(case, 0, 1), case.n_front, 0, False)
    assert want["hits"][0, 0, 0] == (0 if at == "first" else K - 1) and want["hits"][0, 0, 1] == 24 * case.costs[0]
    got = W.demultiplex(dev(case.labels), dev(case.lengths), kit(case), min_fraction=0.0, min_margin=0.0, **kw(case))
    assert_scores(got.scores, ref)
    assert_pick(got, want)
    W.check_device_flags()


def test_kmer_events_of_64_and_65_samples():
    """wave_reduce(+, |) over the lanes that share a long event: one whole round of 64 lanes, and one sample into a second"""
    case = KC._build(14, [[3, 4, 64, 2, 65, 4, 33, 5, 3]], dict(k=5, first=-2))      # first = -2: events 2 .. 6 have a k-mer
    begin, end, events = KC.segments(case, "starts")
    ref = KR.kmer_events_ref(case.signal, case.signal_lengths, case.labels, case.label_lengths, begin, end, events, scale_shift=None,
                             frac_bits=12, max_dwell=255, **case.kw)
    assert ref["length"][0, 2:7].tolist() == [64, 2, 65, 4, 33] and (ref["kmer"][0, 2:7] >= 0).all()
    assert_kmer_events(kmer_events(case, "starts", "f32", 12), ref)
    W.check_device_flags()


# ---- shift and hand-off ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("M", [511, 512, 513])
def test_pairwise_align_across_the_first_wave_seam(M, free):
    """wave_shr1 inside a wave, edge_publish / edge_left between waves 0 and 1: 3 reference rows against one wave and two"""
    rng = np.random.default_rng(M)
    refs = [rng.integers(1, 5, size=3).tolist(), rng.integers(1, 5, size=3).tolist()]
    queries = [rng.integers(1, 5, size=M).tolist(), rng.integers(1, 5, size=M - 1).tolist()[:505] + refs[1] + [1] * (M - 508)]
    assert len(queries[1]) == M
    got = pair_align(refs, queries, PR.EMBOSS, free)
    check_pair_batch(refs, queries, PR.EMBOSS, free, got, "M%d" % M)


@pytest.mark.parametrize("frames", [1, -1])
@pytest.mark.parametrize("L", [255, 256])
def test_forced_align_where_every_frame_advances_one_state(L, frames):
    """L equal labels, so no state is skipped, against 2 L + 1 frames (the end blanks are optional: two frames to
    spare) and against 2 L - 1 frames (the only feasible path starts in the first label and advances one state per frame): every
    value that crosses a lane (wave_shr1) or a wave (edge_publish / edge_left; two waves from 256 labels) decides the result.
    Quarter-grid log-probabilities: every sum is exact"""
    rng = np.random.default_rng(L)
    T = 2 * L + frames
    x = torch.tensor(rng.integers(-24, 1, size=(1, 5, T)) / 4.0, dtype=torch.float32)
    labels = [[2] * L]
    got = forced_align(x, labels, None, input="log_probs")
    check_forced_batch(x, labels, None, got, kind="log_probs", exact=True, tag="L%d" % L)
    states, _, _ = A.viterbi_align(x[0].double().numpy(), labels[0])
    assert frames == 1 or list(states) == list(range(1, T + 1))
