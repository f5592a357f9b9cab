"""CPU: the reference of the indel left-alignment (tests/leftalign_ref.py) against rows worked by hand, against the properties of
every short row (tests/leftalign_cases.py::short_rows) and against the conditions the committed seeds of the repeat-planted run
must meet; and it leaves the two planted runs of tests/pileup_cases.py, which avoid repeats on purpose, as they are."""
from collections import Counter

import numpy as np
import pytest

from tests import leftalign_cases as K
from tests import leftalign_ref as L
from tests import pairwise_align_ref as A
from tests import pileup_cases as C
from tests import pileup_ref as P

A_, G_, C_, T_ = 1, 2, 3, 4


def _check(ops, a, b, want, passes, strand=0, max_passes=8):
    A.replay(a, b, ops)                                              # the hand-made row is an alignment of a and b
    got = L.left_align_row(ops, a, b, strand, max_passes)
    assert got == (want, passes, 1), got
    A.replay(a, b, got[0])


def test_the_two_pass_example():
    """the issue's example (it spells the sequences with five As; the seven ops consume four): pass 1 moves the insertion by one
    and the deletion by two, pass 2 the deletion by one more, next to the insertion"""
    a = b = [C_, A_, A_, A_, A_, G_]
    ops = [1, 1, 4, 1, 1, 3, 1]
    assert L.one_pass(ops, a, b) == ([1, 4, 1, 3, 1, 1, 1], True)
    assert L.one_pass([1, 4, 1, 3, 1, 1, 1], a, b) == ([1, 4, 3, 1, 1, 1, 1], True)
    _check(ops, a, b, [1, 4, 3, 1, 1, 1, 1], 2)
    assert L.left_align_row(ops, a, b, 0, 1) == ([1, 4, 1, 3, 1, 1, 1], 1, 0)
    assert L.left_align_row(ops, a, b, 0, 2) == ([1, 4, 3, 1, 1, 1, 1], 2, 0)        # the last pass that ran still moved
    assert L.left_align_row(ops, a, b, 0, 3) == ([1, 4, 3, 1, 1, 1, 1], 2, 1)
    # on strand 1 the walk is back to front: the mirrored row gives the mirrored result
    assert L.left_align_row(ops[::-1], a[::-1], b[::-1], 1) == ([1, 1, 1, 1, 3, 4, 1], 2, 1)
    # and the row as it stands, walked back to front, moves toward its own end
    assert L.left_align_row(ops, a, b, 1) == ([1, 1, 1, 1, 4, 3, 1], 1, 1)


def test_runs_blocked_by_first_and_by_the_other_gap_type():
    _check([1, 1, 3, 1], [A_, A_, A_, G_], [A_, A_, G_], [1, 3, 1, 1], 1)              # a[0] == a[1] too, but `first` stays
    _check([3, 1, 1, 3, 1], [A_, A_, A_, A_, G_], [A_, A_, G_], [3, 1, 3, 1, 1], 1)    # the leading 3 is an end column
    _check([1, 4, 1, 1, 3, 1], [A_, A_, A_, A_, G_], [A_, C_, A_, A_, G_], [1, 4, 3, 1, 1, 1], 1)
    _check([1, 3, 4, 1], [A_, A_, G_], [A_, A_, G_], [1, 3, 4, 1], 0)                  # side by side: s_max = 0 for the second
    _check([1, 1, 3, 1, 1], [A_, G_, C_, T_, A_], [A_, G_, T_, A_], [1, 1, 3, 1, 1], 0)  # nothing to move
    _check([1, 1, 1, 4, 1, 3], [A_, A_, A_, A_, A_], [A_, A_, A_, A_, A_], [1, 4, 1, 1, 1, 3], 1)   # the trailing 3 is an end column


def test_shifts_shorter_equal_and_longer_than_the_run():
    _check([1, 1, 1, 1, 1, 3, 3, 1], [G_, A_, C_, T_, C_, A_, C_, T_], [G_, A_, C_, T_, C_, T_], [1, 1, 1, 1, 3, 3, 1, 1], 1)     # s = 1 < l
    _check([1, 1, 1, 1, 1, 3, 3, 1], [G_, A_, T_, A_, C_, A_, C_, T_], [G_, A_, T_, A_, C_, T_], [1, 1, 1, 3, 3, 1, 1, 1], 1)     # s = 2 = l
    _check([1, 1, 1, 1, 1, 3, 3, 1], [G_, A_, C_, A_, C_, A_, C_, T_], [G_, A_, C_, A_, C_, T_], [1, 3, 3, 1, 1, 1, 1, 1], 1)     # s = 4 > l
    # a mismatch that the run passes stays a mismatch
    _check([1, 1, 1, 1, 2, 3, 3, 1], [G_, A_, C_, A_, C_, A_, C_, T_], [G_, A_, C_, A_, G_, T_], [1, 3, 3, 1, 1, 1, 2, 1], 1)
    # an insertion is checked on the read: period 2 in b
    _check([1, 1, 1, 1, 1, 4, 4, 1], [G_, A_, C_, A_, C_, T_], [G_, A_, C_, A_, C_, A_, C_, T_], [1, 4, 4, 1, 1, 1, 1, 1], 1)
    # two runs of one kind merge: the first pass brings them side by side, the second moves them as one
    a, b = [G_] + [A_] * 6 + [T_], [G_] + [A_] * 4 + [T_]
    assert L.one_pass([1, 1, 3, 1, 1, 1, 3, 1], a, b) == ([1, 3, 1, 3, 1, 1, 1, 1], True)
    _check([1, 1, 3, 1, 1, 1, 3, 1], a, b, [1, 3, 3, 1, 1, 1, 1, 1], 2)


def test_states_and_batches():
    ops, a, b = [1, 1, 3, 1, 0, 0], [A_, A_, A_, G_, 0], [A_, A_, G_, 0]
    rows = dict(ops=[ops] * 9, ops_len=[4, 4, 4, 4, 7, 4, 4, 4, 4], ref=[a] * 9, ref_lengths=[4, 0, 4, 5, 4, 4, 6, 4, 4], query=[b] * 9,
                query_lengths=[3, 3, 3, 3, 3, 2, 3, 5, 3], strand=[0, 0, -1, 0, 0, 0, 0, 0, 2])
    got = L.left_align_ref(**rows)
    assert got.settled.tolist() == [1, 1, 1, -1, -1, -1, -1, -1, -1] and got.passes.tolist() == [1] + [0] * 8 and got.bad == 6
    assert got.ops[0].tolist() == [1, 3, 1, 1, 0, 0] and all(got.ops[r].tolist() == ops for r in range(1, 9))
    got = L.left_align_ref([[1, 5, 1], [1, 0, 1]], [3, 3], [[1, 1, 1]] * 2, [3, 3], [[1, 1, 1]] * 2, [3, 3], [0, 1])
    assert got.settled.tolist() == [-1, -1] and got.bad == 2


def test_properties_of_every_short_row():
    rows = K.short_rows()
    assert len(rows) == 2 * sum(3 ** n for n in range(1, K.SHORT_MAX + 1))
    most = 0
    for strand in (0, 1):
        after = []
        for ops, a, b in rows:
            out, passes, settled = L.left_align_row(ops, a, b, strand)
            most = max(most, passes)
            assert settled == 1 and Counter(out) == Counter(ops)
            A.replay(a, b, out)                                      # 1 and 2 still agree with the labels
            assert A.rescore(out, *A.EMBOSS, True) >= A.rescore(ops, *A.EMBOSS, True)
            assert L.left_align_row(out, a, b, strand) == (out, 0, 1)                  # the fixed point is one
            mirror = L.left_align_row(ops[::-1], a[::-1], b[::-1], 1 - strand)
            assert (mirror[0][::-1], mirror[1], mirror[2]) == (out, passes, settled)
            after.append(out)
        # the depth per position of a pileup is what it was
        keep = [r for r, (ops, a, b) in enumerate(rows) if a]
        n_ref = [len(rows[r][1]) for r in keep]
        lo = np.concatenate([[0], np.cumsum(n_ref)[:-1]]).astype(int).tolist()
        query, query_len = C.rows([rows[r][2] for r in keep])
        depth = []
        for which in ([rows[r][0] for r in keep], [after[r] for r in keep]):
            ops_rows, ops_len = C.rows(which, dtype=np.uint8)
            pile = P.pileup_ref(ops_rows, ops_len, lo, n_ref, [strand] * len(keep), query, query_len, sum(n_ref))
            assert pile.bad == 0
            depth.append(pile.counts[:, :, :5].sum((1, 2)))
        assert np.array_equal(depth[0], depth[1])
    assert 2 <= most <= 8


@pytest.mark.parametrize("noisy", [False, True])
def test_conditions_of_the_repeat_planted_run(noisy):
    run = K.repeat_planted(noisy)
    assert len(run["records"]) == 10 and sorted(r[1] for r in run["records"]) != ["del"] * 10
    with_, without = K.repeat_host(noisy, True), K.repeat_host(noisy, False)
    # (i) with the left-alignment the chain returns the sample and exactly the planted records
    assert [int(v) for v in with_["calls"].consensus] == run["sample"]
    assert [v[:4] for v in with_["variants"]] == run["records"]
    # (ii) without it the chain fails that (in the error-free run at least; in both with these seeds)
    assert [v[:4] for v in without["variants"]] != run["records"]
    assert [int(v) for v in without["calls"].consensus] != run["sample"]
    # (iii) every read settles within the default max_passes; about half of them change
    aligned = with_["aligned"]
    assert aligned.bad == 0 and aligned.settled.tolist() == [1] * K.PLANT_READS
    assert 10 <= int((aligned.passes > 0).sum()) <= 30
    for r in range(K.PLANT_READS):
        n = int(with_["ops_len"][r])
        window = C.window_labels(run["ref"], *run["window"][r], run["strand"][r])
        A.replay(window, run["reads"][r], [int(v) for v in with_["ops"][r, :n]])
        assert Counter(with_["ops"][r].tolist()) == Counter(with_["raw_ops"][r].tolist())


@pytest.mark.parametrize("noisy", [False, True])
def test_the_planted_runs_without_repeats_stay_as_they_are(noisy):
    run, host = C.planted(noisy), C.planted_host(noisy)
    windows, n_ref = C.rows([C.window_labels(run["ref"], w[0], w[1], s) for w, s in zip(run["window"], run["strand"])])
    got = L.left_align_ref(host["ops"], host["ops_len"], windows, n_ref, run["labels"], run["lengths"], run["strand"])
    assert got.bad == 0 and got.passes.tolist() == [0] * C.PLANT_READS and got.settled.tolist() == [1] * C.PLANT_READS
    assert np.array_equal(got.ops, host["ops"])
