"""CPU: tests/event_align_ref.py, the reference of wn_event_align, held to things it shares no code with: tests/signal_align_ref.py
on single-sample events, the minimum over every path, a sample-by-sample sum of an event's cost, the existence of an alignment
for every (E, N) the moves allow, the tie rule on cases small enough to work by hand -- and the gap the tool closes, on references
alone: reads whose detected events are fewer than their k-mers."""
import itertools

import numpy as np
import pytest

from tests import event_align_cases as C
from tests import event_align_ref as R
from tests import event_detect_ref as D
from tests import signal_align_cases as SC
from tests import signal_align_ref as SA

QMAX = C.QMAX


# ---- 1. one sample per event, stay and step free, no skips: wn_signal_align
@pytest.mark.parametrize("name", ["hand", "homopolymer", "dyadic", "small", "band_never_moves", "moving_band", "cost_clamp", "form_k5_first2"])
def test_single_sample_events_are_signal_align(name):
    case, want = SC.CASES[name], SC.reference(name)
    kw = case.kw
    B, L = case.signal.shape
    n_events = case.signal_lengths.copy()
    ev_starts = np.tile(np.arange(L + 1, dtype=np.int32), (B, 1))
    ev_sum, ev_sumsq = np.zeros((B, L), dtype=np.int64), np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        T = int(case.signal_lengths[b])
        q = np.array(SA.read_samples(case.signal[b], T, None, kw["frac_bits"]), dtype=np.int64)
        ev_sum[b, :T], ev_sumsq[b, :T] = q, q * q
        ev_starts[b, T:] = T
    got = R.event_align_ref(n_events, ev_starts, ev_sum, ev_sumsq, case.labels, case.label_lengths, case.model, (0, 0, -1, -1), k=kw["k"],
                            first=kw["first"], weight_shift=kw["weight_shift"], max_cost=kw["max_cost"], band=kw["band"])
    assert got["bad"] == want["bad"] == 0
    assert got["score"].tolist() == want["score"].tolist()
    assert np.array_equal(got["starts"], want["starts"]) and np.array_equal(got["band_hits"], want["band_hits"])
    assert np.array_equal(got["states"], want["states"])


@pytest.mark.parametrize("S", [16, 32, 63])
def test_an_event_of_one_sample_costs_what_the_sample_costs(S):
    rng = np.random.default_rng(S)
    rows = [(QMAX, -QMAX, (1 << 31) - 1, (1 << 30) - 1, (1 << 31) - 1), (-QMAX, QMAX, (1 << 31) - 1, -(1 << 30) + 1, 12345)]
    assert abs(rows[0][0] - rows[0][1]) == (1 << 24) - 2
    rows += [tuple(int(v) for v in (rng.integers(-QMAX, QMAX + 1), rng.integers(-QMAX, QMAX + 1), rng.integers(1, 1 << 31),
                                    rng.integers(-(1 << 30) + 1, 1 << 30), rng.integers(1, 1 << 31))) for _ in range(2000)]
    for q, level, weight, offset, max_cost in rows:
        assert R.event_cost(1, q, q * q, level, weight, offset, S, max_cost) == SA.sample_cost(q, level, weight, offset, S, max_cost)


# ---- 2. the minimum over every allowed path
def _every_path(E, N, allowed):
    def walk(path):
        if len(path) == E:
            if path[-1] == N - 1:
                yield path
            return
        for m in allowed:
            if path[-1] + m <= N - 1:
                yield from walk(path + [path[-1] + m])
    yield from walk([0])


MOVE_SETS = [tuple(m for m in (0, 1, 2, 3) if m == 1 or m in extra) for r in range(4) for extra in itertools.combinations((0, 2, 3), r)]


def test_the_minimum_over_every_path():
    assert len(MOVE_SETS) == 8 and all(1 in s for s in MOVE_SETS)
    rng = np.random.default_rng(17)
    seen_none = seen_some = 0
    for trial in range(60):
        E, N = int(rng.integers(1, 8)), int(rng.integers(1, 10))
        tie = trial % 3 == 0                                         # a third built to tie: two levels, samples on or between them
        levels = rng.choice([16, 32], size=4) if tie else rng.integers(0, 64, size=4)
        model = np.stack([levels, np.full(4, 1 << 16), rng.integers(-3, 4, size=4) * (0 if tie else 1)], axis=1).astype(np.int64)
        codes = rng.integers(0, 4, size=N).tolist()
        lens = rng.integers(1, 10, size=E)
        q = rng.choice([16, 24, 32], size=int(lens.sum())) if tie else rng.integers(0, 64, size=int(lens.sum()))
        events = R.events_of(q, np.concatenate([[0], np.cumsum(lens)]))
        costs = [8, 8, 8, 8] if tie else rng.integers(0, 50, size=4).tolist()
        for allowed in MOVE_SETS:
            mc = tuple(costs[m] if m in allowed else -1 for m in range(4))
            want = min((R.rescore(events, codes, model, 16, 500, mc, p) for p in _every_path(E, N, allowed)), default=None)
            score, states = R.align_read(events, codes, model, 16, 500, mc, 64)
            assert score == want, (trial, allowed)
            if score is None:
                seen_none += 1
                continue
            seen_some += 1
            assert R.rescore(events, codes, model, 16, 500, mc, states) == score
            assert states[0] == 0 and states[-1] == N - 1 and set(np.diff(states).tolist()) <= set(allowed)
    assert seen_none > 50 and seen_some > 150


# ---- 3. the cost of an event against the sum over its samples
def _by_samples(q, level, weight, offset, S, max_cost):
    return min((sum((int(v) - level) ** 2 for v in q) * weight) >> S, len(q) * max_cost) + len(q) * offset


def test_event_cost_against_a_sample_by_sample_sum():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, 200))
        q = rng.integers(-QMAX, QMAX + 1, size=n) if rng.random() < 0.3 else rng.integers(300000, 500000, size=n)
        level, weight, offset = int(rng.integers(-QMAX, QMAX + 1)), int(rng.integers(1, 1 << 31)), int(rng.integers(-(1 << 30) + 1, 1 << 30))
        S, max_cost = int(rng.integers(16, 64)), int(rng.integers(1, 1 << 31))
        (ev,) = R.events_of(q, [0, n])
        assert R.event_ok(*ev)
        assert R.event_cost(*ev, level, weight, offset, S, max_cost) == _by_samples(q, level, weight, offset, S, max_cost)
    # the largest event: 65536 samples of +-(2^23 - 1) against the level of the other sign, D just under 2^64
    n = 65536
    for sign in (1, -1):
        q = [sign * QMAX] * n
        (ev,) = R.events_of(q, [0, n])
        D_ = n * (2 * QMAX) ** 2
        assert R.event_ok(*ev) and (1 << 63) < D_ < (1 << 64) and D_ == n * ((1 << 24) - 2) ** 2
        for S in (16, 32, 63):
            w = (1 << 31) - 1
            quotient = (D_ * w) >> S
            for max_cost in {1, (1 << 31) - 1, max(quotient // n, 1), quotient // n + 1}:
                got = R.event_cost(*ev, -sign * QMAX, w, 7, S, max_cost)
                assert got == _by_samples(q, -sign * QMAX, w, 7, S, max_cost) == min(quotient, n * max_cost) + 7 * n
    # the clamp on both sides of n max_cost: D = 3 * 100^2, weight 2^16 at S = 16
    ev = (3, 300, 30000)
    assert [R.event_cost(*ev, 0, 1 << 16, 0, 16, mc) for mc in (9999, 10000, 10001)] == [29997, 30000, 30000]
    # and the table's rule: what no samples could have made is refused, the boundary is not
    assert R.event_ok(2, 5, 13) and not R.event_ok(2, 5, 12) and R.event_ok(3, 9, 27) and not R.event_ok(3, 10, 33)
    assert not R.event_ok(0, 0, 0) and not R.event_ok(65537, 0, 0) and not R.event_ok(1, QMAX + 1, (QMAX + 1) ** 2) and not R.event_ok(1, 0, -1)


# ---- 4. an alignment exists exactly where the moves allow one
def test_existence_inside_the_narrowest_band():
    model = SC.HAND_MODEL
    for E in range(1, 41):
        events = [(2, 40, 800)] * E
        for N in range(1, 3 * (E - 1) + 2):
            score, states = R.align_read(events, [1] * N, model, 16, 1000, C.ALL_FREE, 64)
            assert score == 0 and states[-1] == N - 1, (E, N)
        for N in (3 * (E - 1) + 2, 3 * (E - 1) + 5):
            assert R.align_read(events, [1] * N, model, 16, 1000, C.ALL_FREE, 64) == (None, None)
            es = np.arange(0, 2 * E + 1, 2, dtype=np.int32)[None]
            out = R.event_align_ref(np.array([E]), es, np.full((1, E), 40), np.full((1, E), 800), np.full((1, N), 2), np.array([N]), model,
                                    C.ALL_FREE, k=1, weight_shift=16, band=64)
            assert out["score"].tolist() == [R.NO_ALIGNMENT] and out["bad"] == 0 and out["moves"].tolist() == [[0] * 4]
    # the largest move decides: with the double skip forbidden N - 1 <= 2 (E - 1)
    assert R.align_read([(2, 40, 800)] * 5, [1] * 9, model, 16, 1000, (0, 0, 0, -1), 64)[0] == 0
    assert R.align_read([(2, 40, 800)] * 5, [1] * 10, model, 16, 1000, (0, 0, 0, -1), 64) == (None, None)


# ---- 5. ties
def test_the_case_worked_by_hand():
    """levels 10, 20, 30, 40, a sample costs d^2; events (10, 10), (20, 30), (40); moves cost 3, 1, 2, 40.  The middle event in
    state 1: 0 + 100, moves 1 + 2; in state 2: 100 + 0, moves 2 + 1; in state 0 or 3: 500 and the moves 3 + 40: the optimum 103 is
    reached twice, and at the last event the step (from state 2) is tried before the skip (from state 1)"""
    case, ref = C.CASES["hand"], C.reference("hand")
    assert [int(v) for v in ref["score"]] == [103] and ref["states"].tolist() == [[0, 2, 3, -1, -1]]
    assert ref["starts"].tolist() == [[0, 2, 2, 4, 5]] and ref["moves"].tolist() == [[0, 1, 1, 0]] and ref["band_hits"].tolist() == [0]
    events = R.events_of([10, 10, 20, 30, 40], [0, 2, 4, 5])
    mc = case.kw["move_cost"]
    assert [R.rescore(events, [0, 1, 2, 3], case.model, 16, 1 << 30, mc, [0, s, 3]) for s in range(4)] == [543, 103, 103, 543]


def test_ties_on_a_homopolymer_go_to_the_smallest_move():
    """every path costs 0: the stay is taken wherever the state could be reached an event earlier, so the traced path runs ahead by
    three states an event and then stays"""
    ref = C.reference("homopolymer")
    assert [int(v) for v in ref["score"]] == [0, 0, 0]
    for b, E in enumerate((30, 10, 4)):
        assert ref["states"][b, :E].tolist() == [min(3 * e, 9) for e in range(E)]
        assert ref["moves"][b].tolist() == [E - 4, 0, 0, 3]
        assert ref["starts"][b].tolist() == [0, 3, 3, 3, 6, 6, 6, 9, 9, 9, 3 * E]
    # pressed against the band: with a free stay and a step at 1 the same rule walks the band's upper edge
    narrow, wide = C.reference("pressed_w64"), C.reference("pressed_w2048")
    assert int(narrow["band_hits"][0]) > 100 and wide["band_hits"].tolist() == [0] and narrow["score"].tolist() == wide["score"].tolist() == [199]
    assert wide["states"][0, :400].tolist() == [min(e, 199) for e in range(400)]


# ---- 6. the gap: detected events are fewer than k-mers, signal_align has nothing, event_align aligns
def _truth_path(ev_starts, edges, N):
    """each event in the state that holds most of its samples (the smaller state on a tie), ends pinned"""
    states = []
    for s0, s1 in zip(ev_starts[:-1], ev_starts[1:]):
        j0 = int(np.searchsorted(edges, s0, side="right")) - 1
        best, most = j0, -1
        for j in range(j0, N):
            if edges[j] >= s1:
                break
            held = min(s1, edges[j + 1]) - max(s0, edges[j])
            if held > most:
                best, most = j, held
        states.append(best)
    states[0], states[-1] = 0, N - 1
    return states


def _share_in_own_kmer(starts, edges, N):
    """the share of samples that the segmentation `starts` puts into the state the generator drew them from"""
    T = int(edges[-1])
    own = np.repeat(np.arange(N), np.diff(edges))
    got = np.repeat(np.arange(N), np.diff(np.asarray(starts[:N + 1], dtype=np.int64)))
    return float((own == got[:T]).mean())


def test_the_gap_between_detection_and_alignment():
    fx = C.gap_reads()
    B, N, k = C.GAP_READS, C.GAP_STATES, C.GAP_K
    model = C.gap_model(fx)
    det = D.event_detect_ref(fx["signal"], fx["signal_lengths"], D.detectors(frac_bits=C.F), frac_bits=C.F, max_events=256)
    E = det["n_events"]
    assert det["bad"] == 0 and (E < N).all() and (E <= 256).all(), E.tolist()             # the condition on the input
    # the documented pipeline: the event means as a shorter read.  No alignment for any read
    n = np.maximum(np.diff(det["starts"].astype(np.int64), axis=1), 1)
    means = (det["sum"].astype(np.float64) / (n * 2.0 ** C.F)).astype(np.float32)
    sa = SA.signal_align_ref(means, E, fx["labels"], fx["label_lengths"], model, k=k, first=0, frac_bits=C.F, weight_shift=C.S, band=64)
    assert sa["score"].tolist() == [SA.NO_ALIGNMENT] * B and sa["bad"] == 0
    # event_align aligns every read
    out = R.event_align_ref(E, det["starts"], det["sum"], det["sumsq"], fx["labels"], fx["label_lengths"], model, C.MOVES, k=k, first=0,
                            weight_shift=C.S, band=64)
    assert out["bad"] == 0 and all(int(v) < R.INF for v in out["score"])
    illegal = outside = 0
    share = []
    for b in range(B):
        es = [int(v) for v in det["starts"][b, :E[b] + 1]]
        events = [(es[e + 1] - es[e], int(det["sum"][b, e]), int(det["sumsq"][b, e])) for e in range(E[b])]
        codes = SA.read_states(fx["labels"][b], int(fx["label_lengths"][b]), k, 0)
        assert R.rescore(events, codes, model, C.S, (1 << 31) - 1, C.MOVES, out["states"][b, :E[b]]) == int(out["score"][b])
        truth = _truth_path(es, fx["edges"][b], N)
        cost = R.rescore(events, codes, model, C.S, (1 << 31) - 1, C.MOVES, truth)
        if cost is None:
            illegal += 1
        elif any(not R.band_lo(e, N, E[b], 64) <= s < R.band_lo(e, N, E[b], 64) + 64 for e, s in enumerate(truth)):
            outside += 1
        else:
            assert int(out["score"][b]) <= cost
        share.append(_share_in_own_kmer(out["starts"][b], fx["edges"][b], N))
    assert 4 * illegal <= B and outside == 0, (illegal, outside)     # a condition on the input: seed 3 and sigma 1.5 give 2 of 8
    print("share of samples in the generator's own k-mer, per read:", ["%.4f" % s for s in share], "mean %.4f" % np.mean(share))
