"""CPU: tests/demux_ref.py, the reference of wn_demux_scores and wn_demux_pick, held to things it shares no code with: a case worked
by hand, a brute-force enumeration of all semi-global alignments, an infix edit distance, hand-made score tables for the pick, and
the planted run's truth."""
import itertools

import numpy as np

from tests import demux_cases as C
from tests import demux_ref as R

INT_MIN = -2 ** 31


def test_the_case_worked_by_hand():
    """read T A G C T, costs 2 / -2 / 3 / 1.  Front pattern A G C: three matches at [1, 4), 6.  Rear pattern G C A: G C match (4),
    then A against T (-2) = 2 at [2, 5); A against a gap instead gives 4 - 3 = 1; so (2, 2, 5)."""
    ref = C.reference("hand")
    assert ref["score"].tolist() == [[6, 2]] and ref["start"].tolist() == [[1, 2]] and ref["end"].tolist() == [[4, 5]] and ref["bad"] == 0
    # an empty window: every score is -(go + (P - 1) ge), start = end = 0
    assert R.semi_global([1, 2, 3], [], 2, -2, 3, 1) == (-5, 0, 0)
    # a pattern longer than the window: A G C A against G alone, one match and gaps on both sides, the first of them at column 0
    assert R.semi_global([1, 2, 3, 1], [2], 2, -2, 3, 1) == (2 - 3 - 4, 0, 1)


def test_every_small_alignment_against_brute_force():
    """every pattern of length <= 3 over 2 labels against every window of length <= 4: the greatest score over ALL semi-global
    alignments, among those the smallest start, then the smallest end -- under five cost sets, ge = 0, go = ge and free gaps among them"""
    words = lambda nmax, nmin: [list(w) for n in range(nmin, nmax + 1) for w in itertools.product((1, 2), repeat=n)]  # noqa: E731
    checked = 0
    for costs in ((2, -2, 3, 1), (6, -12, 10, 4), (2, -3, 2, 0), (1, -1, 1, 1), (2, -2, 0, 0)):
        for pattern in words(3, 1):
            for window in words(4, 0):
                assert R.semi_global(pattern, window, *costs) == R.all_semi_global(pattern, window, *costs), (costs, pattern, window)
                checked += 1
    assert checked == 5 * 14 * 31


def _infix_distance(p, t):
    """Sellers: the least edit distance of p to any substring of t"""
    col = list(range(len(p) + 1))
    best = col[-1]
    for y in t:
        new = [0]
        for i, x in enumerate(p, 1):
            new.append(min(col[i] + 1, new[i - 1] + 1, col[i - 1] + (x != y)))
        col, best = new, min(best, new[-1])
    return best


def test_unit_costs_give_the_infix_edit_distance():
    rng = np.random.default_rng(3)
    for _ in range(60):
        p = [int(v) for v in rng.integers(1, 4, int(rng.integers(1, 9)))]
        t = [int(v) for v in rng.integers(1, 4, int(rng.integers(0, 15)))]
        assert -R.semi_global(p, t, 0, -1, 1, 1)[0] == _infix_distance(p, t), (p, t)


def _pick(score, group, n_front, min_score, margin=0, both=False, lengths=(100,), start=None, end=None):
    score = np.array([score], dtype=np.int32)
    start = np.zeros_like(score) if start is None else np.array([start], dtype=np.int32)
    end = np.zeros_like(score) if end is None else np.array([end], dtype=np.int32)
    return R.demux_pick_ref(score, start, end, lengths, group, min_score, n_front, margin, both)


def test_pick_rules_on_hand_made_tables():
    # a tie goes to the lower index, at both ends; the runner-up of a tie between groups is the same score
    r = _pick([40, 40, 10, 30, 30], [0, 1, 2, 0, 1], 3, [0] * 5)
    assert r["hits"][0, :, 0].tolist() == [0, 3] and r["runner_up"].tolist() == [[40, 30]] and r["barcode"].tolist() == [0]
    assert _pick([40, 40, 10, 30, 30], [0, 1, 2, 0, 1], 3, [0] * 5, margin=1)["barcode"].tolist() == [-1]
    # the margin counts a different group only: two patterns of one group close together pass, a third group far below
    r = _pick([40, 39, 10], [0, 0, 1], 3, [0] * 3, margin=30)
    assert r["runner_up"].tolist() == [[10, INT_MIN]] and r["barcode"].tolist() == [0] and r["hits"][0, 1].tolist() == [-1] * 4
    assert _pick([40, 39, 10], [0, 0, 1], 3, [0] * 3, margin=31)["barcode"].tolist() == [-1]
    # one group alone: no runner-up, the margin holds; the per-pattern floor decides, on both sides of it
    assert _pick([40, 39], [0, 0], 2, [40, 0], margin=10 ** 6)["barcode"].tolist() == [0]
    assert _pick([40, 39], [0, 0], 2, [41, 0], margin=0)["barcode"].tolist() == [-1]
    # the ends: the passing end with the greater score, a tie to the front; require_both wants both to pass and agree
    table, group = [10, 50, 60, 20], [0, 1, 0, 1]
    assert _pick(table, group, 2, [0] * 4)["barcode"].tolist() == [0]                    # rear 60 beats front 50
    assert _pick([10, 60, 60, 20], group, 2, [0] * 4)["barcode"].tolist() == [1]         # a tie: the front
    assert _pick(table, group, 2, [0, 0, 61, 0])["barcode"].tolist() == [1]              # the rear fails its floor
    assert _pick(table, group, 2, [0, 51, 61, 0])["barcode"].tolist() == [-1]
    assert _pick(table, group, 2, [0] * 4, both=True)["barcode"].tolist() == [-1]        # they disagree
    assert _pick([50, 10, 60, 20], group, 2, [0] * 4, both=True)["barcode"].tolist() == [0]
    assert _pick([50, 10, 60, 20], group, 2, [0, 0, 61, 0], both=True)["barcode"].tolist() == [-1]
    # trims: the front hit's end, the rear hit's start; an end that fails leaves 0 / the length; overlapping trims clamp
    kw = dict(start=[3, 0, 70, 0], end=[27, 0, 94, 0], lengths=(100,))
    assert _pick([50, 10, 60, 20], group, 2, [0] * 4, **kw)["trim"].tolist() == [[27, 70]]
    assert _pick([50, 10, 60, 20], group, 2, [51, 0, 0, 0], **kw)["trim"].tolist() == [[0, 70]]
    assert _pick([50, 10, 60, 20], group, 2, [0, 0, 61, 0], **kw)["trim"].tolist() == [[27, 100]]
    assert _pick([50, 10, 60, 20], group, 2, [0] * 4, start=[3, 0, 20, 0], end=[27, 0, 44, 0])["trim"].tolist() == [[27, 27]]
    # a poisoned entry is no candidate; a poisoned row has no hit at all
    r = _pick([INT_MIN, 10, INT_MIN, INT_MIN], group, 2, [0] * 4)
    assert r["hits"][0].tolist() == [[1, 10, 0, 0], [-1] * 4] and r["barcode"].tolist() == [1] and r["runner_up"].tolist() == [[INT_MIN] * 2]


def test_the_shapes_reach_what_they_are_for():
    """conditions on the cases, from the inputs and the references alone"""
    assert [C.CASES[n].n_front for n in ("k_1_64", "k_63_65", "k_64_63", "front_only", "rear_only")] == [1, 63, 64, 65, 0]
    assert [len(C.CASES[n].group) - C.CASES[n].n_front for n in ("k_1_64", "k_63_65", "k_64_63", "front_only", "rear_only")] == [64, 65, 63, 0, 3]
    for pmax in (8, 9, 32, 33, 64, 65, 96, 97):
        lens = C.CASES["rows_%d" % pmax].pattern_lengths
        assert lens.max() == pmax and lens.min() == 1
    case = C.CASES["p128_w512"]
    assert case.pattern_lengths.tolist() == [128, 5, 128] and case.window == 512 and case.lengths.tolist() == [600]
    ref = C.reference("homopolymer")                                 # every start ties: the smallest start, then the smallest end
    assert ref["start"].tolist() == [[0, 0, 10, 10], [0, 0, 0, 0]] and ref["end"].tolist() == [[5, 1, 15, 16], [4, 1, 4, 4]]
    assert C.reference("costs_limit")["score"][0, 0] == 128 * 1024 and C.CASES["costs_limit"].costs == (1024, -1024, 1024, 1024)
    short = C.CASES["short_reads"]                                   # the windows overlap; rear coordinates are read coordinates
    assert (short.lengths < 2 * short.window).all() and (short.lengths[:3] < short.window).any()
    ref = C.reference("short_reads")
    assert (ref["end"] <= short.lengths[:, None]).all() and (ref["start"] >= 0).all()
    ref = C.reference("longer_than_window")                          # forced gaps; the empty read's scores are the border's
    case = C.CASES["longer_than_window"]
    assert (case.pattern_lengths > case.window).all()
    assert ref["score"][2].tolist() == [-(10 + (int(P) - 1) * 4) for P in case.pattern_lengths] and not ref["start"][2].any() and not ref["end"][2].any()


def test_the_planted_run_is_called_at_its_truth():
    """from the reference alone: the barcode set keeps its distance, and every read with both barcodes planted is called at its true
    group, the best hit of either end being its own pattern; a read missing one end is still called by the other, and trims only that end"""
    p = C.planted()
    codes = p["codes"]
    every = codes + [C.revcomp(c) for c in codes]
    assert min(C.edit_distance(a, b) for i, a in enumerate(every) for b in every[i + 1:]) >= C.PLANT_MIN_DISTANCE
    _, pick = C.planted_reference()
    both = p["has_front"] & p["has_rear"]
    assert both.sum() == C.PLANT_READS - 7
    assert np.array_equal(pick["barcode"][both], p["truth"][both])
    assert np.array_equal(pick["hits"][both, 0, 0], p["truth"][both]) and np.array_equal(pick["hits"][both, 1, 0], p["truth"][both] + C.PLANT_CODES)
    trimmed = (pick["trim"][both, 0] > 0) & (pick["trim"][both, 1] < p["case"].lengths[both])
    assert trimmed.sum() >= 50 and not trimmed.all()                 # a few ends fall below their floor: those stay untrimmed
    assert np.array_equal(pick["barcode"][~both], p["truth"][~both])
    assert (pick["trim"][~p["has_front"], 0] == 0).all() and np.array_equal(pick["trim"][~p["has_rear"], 1], p["case"].lengths[~p["has_rear"]])
