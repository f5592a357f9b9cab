"""CPU: tests/banded_align_ref.py against exhaustive enumeration, against tests/pairwise_align_ref.py (the two properties the GPU
tests rest on) and against hand-worked stripes."""
import itertools

import numpy as np
import pytest

from tests import banded_align_ref as R
from tests import pairwise_align_ref as P
from tests.banded_align_cases import COSTS, random_pair, random_stripe


def _rows(n, m):
    """every op row over n reference and m query labels (a diagonal op stands as a match)"""
    out = []

    def walk(i, j, ops):
        if i == n and j == m:
            out.append(ops)
            return
        if i < n and j < m:
            walk(i + 1, j + 1, ops + [P.OP_MATCH])
        if i < n:
            walk(i + 1, j, ops + [P.OP_REF_GAP])
        if j < m:
            walk(i, j + 1, ops + [P.OP_QUERY_GAP])

    walk(0, 0, [])
    return out


def _diag_cells(ops):
    i = j = 0
    for op in ops:
        if op == P.OP_MATCH:
            yield i, j
        i += op != P.OP_QUERY_GAP
        j += op != P.OP_REF_GAP


@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("costs", [P.EMBOSS, (2, -3, 2, 1)])
def test_exhaustive_enumeration(costs, free):
    """N, M <= 4 over two letters, every stripe from one diagonal outside the rectangle to one outside on the other side: the score
    is the best rescore() over every op row whose path cells lie in the stripe, and there is no alignment iff there is no such row"""
    match, mismatch, go, ge = costs
    for n, m in itertools.product(range(5), repeat=2):
        rows = _rows(n, m)
        gap = np.array([P.rescore(r, 0, 0, go, ge, free) for r in rows])
        on = np.zeros((len(rows), max(n * m, 1)), dtype=np.int64)
        for k, r in enumerate(rows):
            for i, j in _diag_cells(r):
                on[k, i * m + j] = 1
        span = [[j - i for i, j in R.path_cells(r, free)] for r in rows]
        dmin, dmax = np.array([min(d) for d in span]), np.array([max(d) for d in span])
        for a in itertools.product((1, 2), repeat=n):
            for b in itertools.product((1, 2), repeat=m):
                eq = (np.array(a, dtype=np.int64)[:, None] == np.array(b, dtype=np.int64)[None, :]).astype(np.int64).reshape(-1)
                nm = on[:, :n * m] @ eq if n * m else np.zeros(len(rows), dtype=np.int64)
                score = gap + match * nm + mismatch * (on.sum(1) - nm)
                for lo in range(-n - 1, m + 2):
                    for hi in range(lo, m + 2):
                        got = R.align(a, b, lo, hi, match, mismatch, go, ge, free)
                        fits = (dmin >= lo) & (dmax <= hi)
                        if free and n * m == 0:                      # one row of end gaps, whichever border cell is the path
                            fits = np.array([any(lo <= d <= hi for d in range(-n, m + 1))])
                        assert got.status == int(fits.any()), (a, b, lo, hi)
                        if got.status:
                            assert got.score == score[fits].max(), (a, b, lo, hi)
                            assert P.rescore(got.ops, match, mismatch, go, ge, free) == got.score, (a, b, lo, hi)


def _check_row(a, b, lo, hi, costs, free, got):
    """what holds of any result, whatever the reference: the row spells both sequences once, rescores to its score, its counts are
    its op counts, its path cells are in band and edge_hits counts those on the first or last diagonal"""
    ra, rb = P.replay(a, b, got.ops)
    assert ra == list(a) and rb == list(b)
    assert P.rescore(got.ops, *costs, free) == got.score
    assert got.matches == int((got.ops == 1).sum()) and got.mismatches == int((got.ops == 2).sum())
    assert got.gaps == int((got.ops >= 3).sum()) and got.length == len(got.ops)
    if free and len(a) * len(b) == 0:
        return                                                       # a row of end gaps does not say which border cell it was
    cells = R.path_cells(got.ops, free)
    assert all(R.in_band(i, j, lo, hi) for i, j in cells)
    assert got.edge_hits == sum(j - i in (lo, hi) for i, j in cells)


def test_the_two_properties_on_random_pairs():
    rng = np.random.default_rng(71)
    lower = 0
    for trial in range(600):
        letters = (2, 4)[trial % 2]
        costs, free = COSTS[trial % len(COSTS)], bool((trial // 5) % 2)
        n, m = int(rng.integers(0, 15)), int(rng.integers(0, 15))
        a, b = random_pair(rng, n, m, letters, related=trial % 3 != 0)
        full = P.align(a, b, *costs, free)
        # 1: under the stripe of the full path, the full result, ties included
        lo, hi = R.band_from_ops(full.ops, free=free)
        got = R.align(a, b, lo, hi, *costs, free)
        assert got.status == 1 and got[1:6] == full[:5] and np.array_equal(got.ops, full.ops), (a, b, lo, hi)
        _check_row(a, b, lo, hi, costs, free, got)
        wide = R.align(a, b, lo - 1, hi + 1, *costs, free)
        assert np.array_equal(wide.ops, full.ops) and wide.edge_hits == 0
        # 2: under any stripe, at most the full score
        lo, hi = random_stripe(rng, n, m, 6)
        got = R.align(a, b, lo, hi, *costs, free)
        if got.status:
            assert got.score <= full.score
            lower += got.score < full.score
            _check_row(a, b, lo, hi, costs, free, got)
    assert lower > 30                                               # the shifted stripes did bind


def test_whole_matrix_stripe_is_the_full_alignment():
    rng = np.random.default_rng(72)
    for trial in range(200):
        costs, free = COSTS[trial % len(COSTS)], bool(trial % 2)
        n, m = int(rng.integers(0, 20)), int(rng.integers(0, 20))
        a, b = random_pair(rng, n, m, 4, related=trial % 4 != 0)
        full = P.align(a, b, *costs, free)
        for lo, hi in ((-n, m), (-n - 5, m + 7)):
            got = R.align(a, b, lo, hi, *costs, free)
            assert got.status == 1 and got[1:6] == full[:5] and np.array_equal(got.ops, full.ops)


def test_no_alignment_on_both_sides_of_each_bound():
    a, b = [1, 2, 3, 4, 1], [1, 2, 3]                                # N = 5, M = 3: the far corner is on diagonal -2
    c = P.EMBOSS
    assert R.align(a, b, 3, 9, *c, True).status == 1 and R.align(a, b, 4, 9, *c, True).status == 0          # diag_lo > M
    assert R.align(a, b, -9, -5, *c, True).status == 1 and R.align(a, b, -9, -6, *c, True).status == 0      # diag_hi < -N
    assert R.align(a, b, -2, 9, *c, False).status == 1 and R.align(a, b, -1, 9, *c, False).status == 0      # (N, M) below diag_lo
    assert R.align(a, b, -9, -2, *c, False).status == 1 and R.align(a, b, -9, -3, *c, False).status == 0    # above diag_hi
    corner = R.align(a, b, 3, 9, *c, True)                           # only the cell (0, 3): all end gaps
    assert corner.score == 0 and list(corner.ops) == [4, 4, 4, 3, 3, 3, 3, 3] and corner.edge_hits == 1
    none = R.align(a, b, 4, 9, *c, True)
    assert none.score == R.POISON and none.length == 0 and len(none.ops) == 0 and none.edge_hits == 0
    assert R.align([], [], 0, 0, *c, False).status == 1 and R.align([], [], 1, 1, *c, False).status == 0
    assert R.align([], [], 1, 1, *c, True).status == 0 and R.align([], [], -3, 0, *c, True).length == 0


def test_band_from_ops_by_hand():
    B = R.band_from_ops
    assert B([1, 1, 1]) == (0, 0)
    assert B([4, 4, 1, 1, 3, 1]) == (1, 2)                           # starts in (0, 2); the ref gap steps down to diagonal 1
    assert B([3, 1, 4, 4, 2, 3, 3]) == (-1, 1)                       # the trailing 3 3 are end gaps: the path ends on diagonal 1
    assert B([3, 1, 4, 4, 2, 3, 3], free=False) == (-1, 1)           # penalised: they are path, down to diagonal -1
    assert B([1, 4, 4, 2, 3, 3, 3], free=False) == (-1, 2)
    assert B([1, 4, 4, 2, 3, 3, 3], free=True) == (0, 2)
    assert B([4, 4, 4]) == (3, 3) and B([3, 3]) == (-2, -2)          # end gaps only: the one cell before column h
    assert B([4, 4, 4], free=False) == (3, 3)
    assert B([]) == (0, 0)                                           # both lengths zero
    assert B([4, 4, 3, 3, 3]) == (2, 2)                              # (0, 2), then a tail of end gaps
    assert B([4, 4, 3, 3, 3], free=False) == (-1, 2)
    assert B([1, 1], margin=3) == (-3, 3)
    assert B([1, 4, 4, 4, 4, 1], margin=1, max_band=4) == (0, 3)     # [-1, 5] is 7 wide: clamped about its centre
    assert B([1, 4, 4, 4, 4, 1], margin=1, max_band=7) == (-1, 5)
    assert R.path_cells([4, 1, 3, 4], True) == [(0, 1), (1, 2), (2, 2)]
    assert R.path_cells([4, 1, 3, 4], False) == [(0, 1), (1, 2), (2, 2), (2, 3)]
