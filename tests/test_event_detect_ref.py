"""CPU: the reference of the event detection (tests/event_detect_ref.py) against a brute-force restatement in sorted Fractions, and
the proof, from the reference alone, that every case of tests/event_detect_cases.py reaches what it is for: the noise-free reads
give back their change points, the square wave its first edge (and the two comparisons of the peak rule cannot be swapped), the
wide case compares 128-bit products on both sides of bit 64, the merge rule drops at w_1 and keeps at w_1 + 1, and the chain raw
read -> events -> signal_map -> signal_align finds its loci on reads whose bases nobody supplied."""
from fractions import Fraction

import numpy as np
import pytest

from tests import event_detect_cases as C
from tests import event_detect_ref as R
from tests.signal_align_ref import read_samples


def brute_force(q, dets, max_event_len):
    """the definition restated: scores as Fractions, a peak by sorting its neighbourhood"""
    T = len(q)

    def peaks(det):
        w, r = det.window, det.radius
        score = [Fraction(0)] * (T + 1)
        for i in range(w, T - w + 1):
            s1, s2 = sum(q[i - w:i]), sum(q[i:i + w])
            var = w * sum(v * v for v in q[i - w:i + w]) - s1 * s1 - s2 * s2
            score[i] = Fraction(w * (s2 - s1) ** 2, max(var, det.vmin))
        out = []
        for i in range(T + 1):
            hood = sorted(range(max(i - r, 0), min(i + r, T) + 1), key=lambda j: (-score[j], j))     # best first, ties to the smaller
            if hood[0] == i and score[i] * 256 >= det.threshold:
                out.append(i)
        return out

    short = peaks(dets[0])
    long_ = [p for p in peaks(dets[1]) if all(abs(p - s) > dets[1].window for s in short)] if dets[1].window else []
    kinds = {p: 2 for p in long_}
    kinds.update({p: 1 for p in short})
    kinds[0] = 0
    cuts, out = sorted(kinds) + [T], []
    for a, b in zip(cuts, cuts[1:]):
        out += [(a, kinds[a])] + [(a + k * max_event_len, 3) for k in range(1, (b - a - 1) // max_event_len + 1)]
    return out


@pytest.mark.parametrize("seed", range(6))
def test_reference_against_brute_force(seed):
    """T <= 60, small integers so that ties are common, every combination of windows, radii and a small max_event_len"""
    rng = np.random.default_rng(seed)
    for T in (1, 2, 5, 6, 7, 13, 30, 60):
        q = [int(v) for v in np.repeat(rng.integers(-4, 5, size=T), rng.integers(1, 5, size=T))[:T] + rng.integers(-1, 2, size=T)]
        w0, w1 = int(rng.integers(1, 5)), int(rng.integers(0, 7))
        dets = (R.Detector(w0, int(rng.integers(1, 9)), int(rng.integers(1, 2000)), int(rng.integers(1, 40))),
                R.Detector(w1, int(rng.integers(1, 9)), int(rng.integers(1, 2000)), int(rng.integers(1, 40))))
        M = int(rng.integers(1, 12))
        assert R.boundaries_of(q, dets, M) == brute_force(q, dets, M), (seed, T, dets, M)


def test_outputs_of_the_reference():
    """the table around the boundaries: truncation keeps the true count and whole events, the rest follows the convention"""
    full, cut = C.reference("lengths"), C.reference("truncated")
    case = C.CASES["lengths"]
    assert np.array_equal(full["n_events"], cut["n_events"]) and int(full["n_events"].max()) > 7
    assert full["n_events"].tolist()[:2] == [0, 1] and full["bad"] == 0
    for b, T in enumerate(case.signal_lengths):
        n = int(full["n_events"][b])
        q = read_samples(case.signal[b], int(T), None, 12)
        assert (full["starts"][b, n:] == T).all() and (full["kind"][b, n:] == -1).all() and not full["sum"][b, n:].any()
        assert sum(full["sum"][b]) == sum(q) and sum(full["sumsq"][b]) == sum(v * v for v in q)      # the events tile the read
        m = min(n, 7)
        assert np.array_equal(cut["starts"][b, :m + 1], full["starts"][b, :m + 1]) and list(cut["sum"][b, :m]) == list(full["sum"][b, :m])
    assert C.reference("bad")["bad"] == len(C.BAD_READS) - len(C.BAD_GOOD) == 7


@pytest.mark.parametrize("seed", range(20))
def test_noise_free_recovery(seed):
    """dwells in 13..39 (at least 2 w_1 + 1), levels at least 1 apart, min_var 0.01: exactly the true change points, all short"""
    rng = np.random.default_rng(1000 + seed)
    levels = [90.0]
    while len(levels) < 25:
        v = round(90.0 + 12.0 * rng.standard_normal(), 2)
        if abs(v - levels[-1]) >= 1.0:
            levels.append(v)
    x, edges = C.steps(levels, rng.integers(13, 40, size=25))
    q = read_samples(x.astype(np.float32), len(x), None, 12)
    dets = C.detectors_of(C.DEFAULT_KW)
    assert dets[0].vmin == round(0.01 * 4 ** 12 * 9) and dets[1].vmin == round(0.01 * 4 ** 12 * 36)
    assert R.boundaries_of(q, dets) == [(0, 0)] + [(e, 1) for e in edges]


@pytest.mark.parametrize("name", ["noise_free", "seams", "halo", "merge", "ties", "forced_small", "forced_large"])
def test_cases_reach_their_truth(name):
    ref, case = C.reference(name), C.CASES[name]
    assert ref["bad"] == 0
    for b, want in enumerate(case.truth):
        assert C.boundaries(ref, b) == want, (name, b)
    if name == "forced_large":
        assert ref["sumsq"][0, 0] == 65536 * C.QMAX ** 2 > 2 ** 61 and ref["sum"][1, 1] == -65536 * C.QMAX and ref["sum"][0, 2] == 3 * C.QMAX


@pytest.mark.parametrize("M", [64, 5])
def test_forced_gaps_are_long_enough(M):
    """more than 16 forced splits before the step at 1500 and before the end of the constant read; at 5, splits inside a word"""
    ref = C.reference("forced_gap_%d" % M)
    first, flat = C.boundaries(ref, 0), C.boundaries(ref, 3)
    assert first[:1499 // M + 2] == [(0, 0)] + [(k * M, 3) for k in range(1, 1499 // M + 1)] + [(1500, 1)] and 1499 // M > 16
    assert flat == [(0, 0)] + [(k * M, 3) for k in range(1, 999 // M + 1)]
    kinds = [k for _, k in C.boundaries(ref, 1)]
    assert kinds.count(1) > 20 and (kinds.count(3) > 20) == (M == 5)


@pytest.mark.parametrize("M", [1, 2, 3])
def test_dense_cases_hold_long_gaps_inside_words(M):
    """per 1024-word step: the gaps that lie inside one 64-position word and hold more than 16 forced splits.  At max_event_len 1
    there are more of them than a workgroup has threads; at 2 and 3 such a gap needs 35 and 52 of a word's 64 positions, so
    about a half and an eighth of the 1750 and 1170 gaps of a step qualify: hundreds, and at least a hundred"""
    ref = C.reference("dense_%d" % M)
    assert ref["bad"] == 0 and C.DENSE_T > 1024 * 64
    worst = 0
    for b in range(3):
        natural = [p for p, k in C.boundaries(ref, b) if k != 3]
        inside = [p for a, p in zip(natural, natural[1:]) if a // 64 == p // 64 and (p - a - 1) // M > 16]
        worst = max(worst, sum(1 for p in inside if p < 65536))
        assert all((p - a - 1) // M <= 62 for a, p in zip(natural, natural[1:]) if a // 64 == p // 64)
    assert worst > {1: 1024, 2: 300, 3: 100}[M], worst


def test_ties_go_to_the_first_edge_and_the_comparisons_cannot_be_swapped():
    case = C.CASES["ties"]
    q = read_samples(case.signal[0], int(case.signal_lengths[0]), None, 0)
    dets = C.detectors_of(case.kw)
    sc = R.scores(q, dets[0])
    edges = list(range(C.TIE_FIRST, len(q) - 3 + 1, C.TIE_HALF))           # up to T - w
    assert len(edges) > 30 and 2 * C.TIE_HALF <= dets[0].radius
    assert len({Fraction(*sc[e]) for e in edges}) == 1 and all(R.passes(sc[e], dets[0]) for e in edges)       # every edge ties
    assert R.peaks_of(sc, dets[0]) == [C.TIE_FIRST]
    swapped = R.peaks_of(sc, dets[0], left=lambda x, y: x >= y, right=lambda x, y: x > y)
    assert swapped == [edges[-1]]                                    # >= on the left, > on the right: the last edge instead
    assert R.peaks_of(sc, dets[0], left=lambda x, y: x >= y) == edges                # >= on both sides: every edge
    assert R.peaks_of(sc, dets[0], right=lambda x, y: x > y) == []                   # > on both sides: none


def test_the_comparator_needs_all_128_bits():
    case = C.CASES["width"]
    dets = C.detectors_of(case.kw)
    assert dets[0].window == 16 and dets[0].vmin == 1
    q = read_samples(case.signal[0], int(case.signal_lengths[0]), None, 0)
    assert max(q) == C.QMAX and min(q) == -C.QMAX
    sc = R.scores(q, dets[0])
    assert 2 ** 59 < max(a for a, _ in sc) < 2 ** 60 and 2 ** 54 < max(v for _, v in sc) <= 2 ** 55
    log = []
    peaks = R.peaks_of(sc, dets[0], compare_log=log)
    low = (1 << 64) - 1
    below = [(x, y) for x, y in log if x != y and x >> 64 == y >> 64]
    above = [(x, y) for x, y in log if x != y and x & low == y & low]
    assert below and above and any(x == y for x, y in log)
    assert any(x >> 64 for x, _ in below)                            # ... some of them beyond 64 bits with equal high halves
    assert max(max(x, y) for x, y in log) > 2 ** 112
    # a comparator that drops the high half finds other peaks; one that drops the low half decides some comparisons otherwise
    wrong = R.peaks_of(sc, dets[0], left=lambda x, y: x & low > y & low, right=lambda x, y: x & low >= y & low)
    assert wrong != peaks and len(peaks) == 2
    assert any((x > y) != (x >> 64 > y >> 64) for x, y in log)
    assert [p for p, _ in C.boundaries(C.reference("width"), 0)][1:] == peaks


def test_merge_rule_distance():
    case = C.CASES["merge"]
    dets = C.detectors_of(case.kw)
    for b, gap in enumerate((C.MERGE_W1, C.MERGE_W1 + 1)):
        q = read_samples(case.signal[b], int(case.signal_lengths[b]), None, 0)
        short, long_ = R.peaks_of(R.scores(q, dets[0]), dets[0]), R.peaks_of(R.scores(q, dets[1]), dets[1])
        assert short == [100] and long_ == [100, 100 + gap]          # the long peak is there both times; only the merge rule differs
    assert C.reference("merge")["n_events"].tolist() == [2, 3]


def test_seam_cases_lie_on_the_seam():
    ref = C.reference("seams")
    firsts = [C.boundaries(ref, b)[1] for b in range(5)]
    assert firsts == [(256, 1), (255, 1), (257, 1), (250, 1), (249, 2)]
    assert C.boundaries(ref, 3)[2] == (262, 2) and C.boundaries(ref, 4)[2] == (263, 1)
    assert C.CHUNK == 256


def test_composition_on_the_cpu():
    """raw reads -> events -> map -> align with the references alone: one event per state, the true locus is the unique optimum of
    the mapping, and the alignment of the event means to the mapped span gives every state exactly one event"""
    from tests import signal_align_ref as AR
    from tests import signal_map_ref as MR
    from wavenet_speech_amd import signal_model
    fx = C.composition()
    kw = fx["kw"]
    ev = R.event_detect_ref(fx["signal"], fx["signal_lengths"], C.detectors_of(kw), kw["frac_bits"], kw["max_event_len"], kw["max_events"])
    assert ev["bad"] == 0 and ev["n_events"].tolist() == [C.COMPOSE_STATES] * 4
    assert np.array_equal(ev["starts"][:, 1:C.COMPOSE_STATES + 1], np.cumsum(fx["dwells"], axis=1))
    n = C.COMPOSE_STATES
    length = np.diff(ev["starts"][:, :n + 1].astype(np.int64), axis=1)
    means = np.zeros((4, kw["max_events"]), dtype=np.float32)
    means[:, :n] = (ev["sum"][:, :n].astype(np.float64) / (length * 4096.0)).astype(np.float32)
    model = signal_model(fx["means"], fx["stdvs"], frac_bits=C.COMPOSE_F)
    table = model.table.numpy()
    hit = MR.signal_map_ref(means, ev["n_events"], fx["joined"], table, C.COMPOSE_K, C.COMPOSE_F, model.weight_shift)
    assert hit["bad"] == 0 and hit["start"].tolist() == fx["start_state"].tolist()
    assert (hit["end"] - hit["start"] == n - 1).all() and (hit["runner_up"] > hit["score"]).all()
    assert [MR.strand_of(int(e), 2000) for e in hit["end"]] == fx["strand"].tolist()
    for b in range(4):
        s = int(hit["start"][b])
        labels = fx["joined"][s:s + n + C.COMPOSE_K - 1]
        codes = AR.read_states(labels, len(labels), C.COMPOSE_K, 0)
        q = AR.read_samples(means[b], n, None, C.COMPOSE_F)
        score, states = AR.align_read(q, codes, table, model.weight_shift, 2 ** 31 - 1, None)
        assert list(states) == list(range(n)) and score == int(hit["score"][b])
