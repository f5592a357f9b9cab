"""CPU: the forced-alignment reference of tests/ctc_align_ref.py against exhaustive enumeration, the CTC oracle (the best
alignment is one term of the sum the loss takes), its own outputs' consistency, and a hand-made case that pins the tie rule."""
import numpy as np
import pytest

from oracle import ctc_oracle as CO
from tests import ctc_align_ref as A


def _case(seed, C, T, L):
    rng = np.random.default_rng(seed)
    lp = A.log_softmax(rng.normal(size=(C, T)) * 1.5)
    labels = rng.integers(1, C, size=L).tolist()
    return lp, labels


@pytest.mark.parametrize("C,T,L", [(3, 5, 2), (3, 6, 3), (4, 5, 1), (3, 4, 0), (3, 6, 2)])
@pytest.mark.parametrize("seed", range(5))
def test_reference_equals_enumeration(C, T, L, seed):
    lp, labels = _case(100 * seed + 7 * C + T + L, C, T, L)
    states, score, spans = A.viterbi_align(lp, labels)
    want = A.best_score_by_enumeration(lp, labels)
    if np.isneginf(want):
        assert np.isneginf(score) and (states == -1).all() and (spans == -1).all()
        return
    assert abs(score - want) < 1e-12
    assert abs(A.path_score(lp, labels, states) - want) < 1e-12
    assert A.collapse(A.frame_labels_of(states, labels)) == labels


def test_infeasible_is_minus_infinity_in_both():
    rng = np.random.default_rng(0)
    lp = A.log_softmax(rng.normal(size=(3, 4)))
    for labels in ([1, 1, 1], [1, 2, 1, 2, 1], [2, 2, 1, 2]):       # 3 + 2 repeats, 5 labels, 4 + 1 repeat: more than 4 frames
        states, score, spans = A.viterbi_align(lp, labels)
        assert np.isneginf(score) and np.isneginf(A.best_score_by_enumeration(lp, labels))
        assert (states == -1).all() and (spans == -1).all()
    assert A.viterbi_align(lp[:, :0], [])[1] == 0.0 and np.isneginf(A.viterbi_align(lp[:, :0], [1])[1])


@pytest.mark.parametrize("seed", range(4))
def test_score_is_bounded_by_the_loss(seed):
    rng = np.random.default_rng(seed)
    C, T, L = 5, 40, 9
    x = rng.normal(size=(C, T)) * 1.5
    labels = rng.integers(1, C, size=L).tolist()
    nll, _ = CO.ctc_nll_and_grad(x, labels)
    states, score, spans = A.viterbi_align(A.log_softmax(x), labels)
    assert score <= -nll and score > -nll - T * np.log(3.0)          # one of at most 3^T alignments
    fl = A.frame_labels_of(states, labels)
    assert A.collapse(fl) == labels
    for j, (lo, hi) in enumerate(spans):
        assert (fl[lo:hi] == labels[j]).all() and (states[lo:hi] == 2 * j + 1).all()
        assert (lo == 0 or states[lo - 1] != 2 * j + 1) and (hi == T or states[hi] != 2 * j + 1)
    assert (A.frame_margins(A.log_softmax(x), labels, states) >= 0).all()


def test_margins_are_gaps_to_the_best_other_path():
    lp, labels = _case(3, 3, 6, 2)
    states, score, _ = A.viterbi_align(lp, labels)
    margins = A.frame_margins(lp, labels, states)
    ext = A.extended(labels, 0)
    legal = []
    for path in np.ndindex(*([len(ext)] * 6)):                      # every state sequence; the legal ones are scored
        try:
            legal.append((path, A.path_score(lp, labels, path)))
        except AssertionError:
            pass
    assert max(v for _, v in legal) == pytest.approx(score, abs=1e-12)
    for t in range(6):
        other = max(v for path, v in legal if path[t] != states[t])
        assert abs((score - other) - margins[t]) < 1e-12


def test_the_tie_rule():
    """all log-probabilities equal: every alignment scores the same, so the path is decided by the tie rule alone.  labels (1, 2),
    l' = (0, 1, 0, 2, 0), T = 4: the end is state 4 (S - 1 unless S - 2 is strictly better); staying wins wherever the state was
    reachable a frame earlier (frame 3 -> 2 in state 4), else the nearest predecessor: state 4 at frame 2 comes from 3 (state 4
    is not reachable at frame 1), state 3 at frame 1 from state 1 by the skip (states 3 and 2 are not reachable at frame 0)."""
    lp = np.zeros((3, 4))
    states, score, spans = A.viterbi_align(lp, [1, 2])
    assert score == 0.0
    assert states.tolist() == [1, 3, 4, 4]
    assert A.frame_labels_of(states, [1, 2]).tolist() == [1, 2, 0, 0]
    assert spans.tolist() == [[0, 1], [1, 2]]
    assert (A.frame_margins(lp, [1, 2], states) == 0).all()
    # a repeated label forbids the skip: (1, 1) in 4 frames under the same rule
    states, score, spans = A.viterbi_align(lp, [1, 1])
    assert states.tolist() == [1, 2, 3, 4] and spans.tolist() == [[0, 1], [2, 3]]
    # strictly better last label: the path ends in S - 2
    lp = np.zeros((3, 3))
    lp[0, 2] = -1.0
    states, score, _ = A.viterbi_align(lp, [2])
    assert states.tolist() == [1, 1, 1] and score == 0.0
