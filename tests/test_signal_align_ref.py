"""CPU: the reference of signal_align (tests/signal_align_ref.py) held to things it shares no code with: an exhaustive enumeration
of every segmentation, a case worked by hand, the tie rule, Python integers for the 128-bit cost, and the band's identities."""
import itertools
import random

import numpy as np
import pytest

from tests import signal_align_cases as C
from tests import signal_align_ref as R


def _enumerate_min(q, codes, model, S, max_cost):
    """the cheapest of all C(T - 1, N - 1) segmentations, each costed sample by sample"""
    T, N = len(q), len(codes)
    best = None
    for cuts in itertools.combinations(range(1, T), N - 1):
        starts = (0,) + cuts + (T,)
        cost = R.rescore(q, codes, model, S, max_cost, starts)
        best = cost if best is None or cost < best else best
    return best


def test_minimum_equals_exhaustive_enumeration():
    rng = random.Random(5)
    n_tied = 0
    for trial in range(120):
        T, N = rng.randint(1, 9), rng.randint(1, 5)
        if N > T:
            T, N = N, T
        tying = trial % 3 == 0                                       # a coarse table and coarse samples: many equal costs
        model = np.array([[rng.choice([0, 4]) if tying else rng.randint(-50, 50), (1 << 16) * rng.randint(1, 3), rng.randint(-3, 3) * (not tying)]
                          for _ in range(4)], dtype=np.int64)
        q = [rng.choice([0, 2, 4]) if tying else rng.randint(-60, 60) for _ in range(T)]
        codes = [rng.randrange(4) for _ in range(N)]
        max_cost = rng.choice([7, 100, 2 ** 31 - 1])
        score, states = R.align_read(q, codes, model, 16, max_cost, None)
        assert score == _enumerate_min(q, codes, model, 16, max_cost), (trial, q, codes)
        starts = R.starts_of(states, N, T, N)
        assert R.rescore(q, codes, model, 16, max_cost, starts) == score          # the path costs what it claims
        assert states[0] == 0 and states[-1] == N - 1 and set(np.diff(states).tolist()) <= {0, 1}
        banded, _ = R.align_read(q, codes, model, 16, max_cost, 64)               # a band wider than the read changes nothing
        assert banded == score
        n_tied += tying
    assert n_tied == 40


def test_the_case_worked_by_hand():
    """levels 10, 20, 30, cost d^2, samples 10 14 16 20 26 30: [10 14 | 16 20 | 26 30] costs 0 + 16 + 16 + 0 + 16 + 0 = 48; moving
    16 into the first state costs 36 instead of 16, moving 14 or 26 across likewise"""
    ref = C.reference("hand")
    assert ref["score"].tolist() == [48] and ref["bad"] == 0
    assert ref["starts"].tolist() == [[0, 2, 4, 6]]
    assert ref["states"].tolist() == [[0, 0, 1, 1, 2, 2, -1]]
    assert ref["band_hits"].tolist() == [0]


def test_ties_go_to_the_stay():
    ref = C.reference("homopolymer")
    assert ref["states"][0, :30].tolist() == list(range(10)) + [9] * 20
    assert ref["states"][1, :10].tolist() == list(range(10)) and (ref["states"][1, 10:] == -1).all()
    assert ref["starts"][0].tolist() == list(range(10)) + [30]
    assert ref["score"].tolist() == [0, 0]
    # the dyadic table: the optimum is shared by other segmentations (found by moving one boundary), the rule picks one
    case, ref = C.CASES["dyadic"], C.reference("dyadic")
    shared = 0
    for b in range(3):
        T = int(case.signal_lengths[b])
        q = R.read_samples(case.signal[b], T, None, 0)
        codes = R.read_states(case.labels[b], 50, 1, 0)
        starts = ref["starts"][b].tolist()
        for j in range(1, 50):
            for move in (-1, 1):
                other = list(starts)
                other[j] += move
                if other[j - 1] < other[j] < other[j + 1]:
                    cost = R.rescore(q, codes, case.model, 16, 2 ** 31 - 1, other)
                    assert cost >= ref["score"][b]
                    shared += cost == ref["score"][b]
    assert shared > 10


def test_cost_in_full_width_and_the_clamp():
    d, w = 2 ** 24 - 1, 2 ** 31 - 1
    for S in (16, 32, 63):
        want = (d * d * w) >> S
        assert want >= 2 ** 15                                       # the product has 79 bits
        for level, q in ((0, d), (d, 0), (2 ** 23 - 1, -2 ** 23), (-2 ** 23 + 1, 2 ** 23 - 1)):
            if abs(q - level) != d:
                continue
            got = R.cost_row(q, np.array([level]), np.array([w]), np.array([-5]), S, 2 ** 31 - 1)
            assert int(got[0]) == min(want, 2 ** 31 - 1) - 5 == R.sample_cost(q, level, w, -5, S, 2 ** 31 - 1)
    assert R.sample_cost(d, 0, w, 0, 63, 2 ** 31 - 1) == (d * d * w) >> 63 == 65535                   # below the clamp: the shift itself
    assert int(R.cost_row(d, np.array([0]), np.array([w]), np.array([0]), 63, 2 ** 31 - 1)[0]) == 65535
    assert R.sample_cost(100, 0, 1 << 16, 9, 16, 9999) == 9999 + 9 and R.sample_cost(100, 0, 1 << 16, 9, 16, 10000) == 10000 + 9
    assert R.sample_cost(100, 0, 1 << 16, 9, 16, 10001) == 10000 + 9
    rng = random.Random(9)
    for _ in range(3000):                                            # the numpy row against Python integers
        S = rng.randint(16, 63)
        q, level = rng.randint(-2 ** 23 + 1, 2 ** 23 - 1), rng.randint(-2 ** 23 + 1, 2 ** 23 - 1)
        if rng.random() < 0.5:
            level = q + rng.randint(-3000, 3000)
            level = max(min(level, 2 ** 23 - 1), -2 ** 23 + 1)
        weight, offset = rng.randint(1, 2 ** 31 - 1), rng.randint(-2 ** 30 + 1, 2 ** 30 - 1)
        max_cost = rng.choice([1, 1000, 2 ** 20, 2 ** 31 - 1])
        got = R.cost_row(q, np.array([level]), np.array([weight]), np.array([offset]), S, max_cost)
        assert int(got[0]) == R.sample_cost(q, level, weight, offset, S, max_cost), (q, level, weight, S)


@pytest.mark.parametrize("W", [64, 128, 2048])
def test_band_identities(W):
    for T in (1, W + 3, 3 * W + 1, 5000):
        for N in sorted({1, W - 1, W, W + 1, T} & set(range(1, T + 1))):
            c = [R.band_centre(t, N, T) for t in range(T)]
            lo = [R.band_lo(t, N, T, W) for t in range(T)]
            assert c[0] == 0 and c[-1] == N - 1 and lo[0] == 0
            assert set(np.diff(c).tolist()) <= {0, 1} and set(np.diff(lo).tolist()) <= {0, 1}
            assert all(l <= x < l + W and 0 <= l and x < N for l, x in zip(lo, c))          # the centre line is a path in the band
            assert lo[-1] == max(N - W, 0)


def test_no_alignment_and_bad_reads_in_the_reference():
    ref = C.reference("small")
    assert ref["bad"] == 0
    assert ref["score"].tolist()[2:] == [R.NO_ALIGNMENT] * 4 and ref["band_hits"].tolist() == [0] * 6
    assert (ref["starts"][2:] == -1).all() and (ref["states"][2:] == -1).all()
    assert ref["starts"][0].tolist()[:2] == [0, 5] and ref["states"][1, :7].tolist() == list(range(7))
    bad = C.bad_reference()
    want = [name not in C.BAD_GOOD for name in C.BAD_READS]
    assert [s == R.BAD_READ for s in bad["score"].tolist()] == want and bad["bad"] == sum(want)
    assert (bad["starts"][want] == -1).all() and (bad["band_hits"][want] == -1).all()
    for seed in (1, 2):
        g = C.call_ref(C.garbage_batch(seed))
        assert g["bad"] > 12


def test_the_cases_hold_what_they_are_for():
    assert C.reference("band_never_moves")["score"].tolist() == C.call_ref(C.CASES["band_never_moves"], band=None)["score"].tolist()
    moving = C.CASES["moving_band"]
    assert int(moving.label_lengths[0]) - 4 - 4 == 300 and 300 / 64 > 4                      # every slot is used more than four times
    tight, wide = C.reference("pressed_w64"), C.reference("pressed_w2048")
    assert tight["band_hits"][0] > 0 and wide["band_hits"][0] == 0 and wide["score"][0] <= tight["score"][0]
    clamp = C.CASES["cost_clamp"]
    free = C.call_ref(clamp._replace(kw=dict(clamp.kw, max_cost=None)))
    assert (free["score"] > C.reference("cost_clamp")["score"] + 10 ** 6).all()
    long_read = C.CASES["long_read"]
    assert long_read.signal_lengths[0] > 65536 and long_read.label_lengths[0] - 4 == 9000
