"""CPU: the plain-Python CTC decoders of tests/ctc_decode_ref.py (the reference the GPU decoders are held to, test_gpu_decode.py)
against ground truth -- exact enumeration of every alignment, the CTC loss oracle as an upper bound, argmax + collapse -- and the
host-side pieces of wavenet_speech_amd.decoding (argument checks, string helpers) that run without a GPU.  Also the tie-group
matcher of ctc_decode_ref (what it accepts and what it rejects) and, on the reference alone, the conditions the inputs of
test_gpu_decode_edges.py (tests/ctc_decode_cases.py) must meet: at least 90 % of the finite beams of every case are checked."""
import numpy as np
import pytest
import torch

from oracle import ctc_oracle as CO
from tests import ctc_decode_cases as K
from tests import ctc_decode_ref as R


def _exact_order(exact):
    return sorted(exact.items(), key=lambda kv: -kv[1])


def _nll(x, labels, blank=0):
    lab = np.array([list(labels) or [blank + 1]])
    return CO.ctc_total(np.asarray(x, dtype=np.float64)[None], lab, np.array([len(labels)]), blank)[0]


@pytest.mark.parametrize("C,T", [(3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (4, 1), (4, 2), (4, 3)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_beam_is_exact_when_nothing_is_pruned(C, T, kind):
    rng = np.random.default_rng(100 * C + T)
    logits = rng.normal(size=(C, T)) * 1.5
    x = {"logits": logits, "probs": np.exp(R.log_probs(logits)), "log_probs": R.log_probs(logits)}[kind]
    exact = R.exact_labelling_log_probs(logits)
    assert len(exact) <= 64
    beams = R.beam_decode(x, 64, kind=kind)
    want = _exact_order(exact)
    assert [b[0] for b in beams] == [l for l, _ in want]           # every labelling, in the exact order
    for (l, fr, s), (_, v) in zip(beams, want):
        assert abs(s - v) < 1e-9, (l, s, v)
        assert len(fr) == len(l) and all(0 <= f < T for f in fr) and list(fr) == sorted(set(fr))


@pytest.mark.parametrize("blank", [0, 2])
def test_beam_is_exact_with_another_blank(blank):
    rng = np.random.default_rng(7)
    x = rng.normal(size=(3, 5)) * 2.0
    exact = R.exact_labelling_log_probs(x, blank=blank)
    beams = R.beam_decode(x, 64, blank=blank)
    assert [b[0] for b in beams] == [l for l, _ in _exact_order(exact)]
    assert max(abs(s - exact[l]) for l, _, s in beams) < 1e-9


@pytest.mark.parametrize("W", [1, 2, 4, 8])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pruned_beams_are_lower_bounds_of_the_ctc_probability(W, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(5, 14)) * 1.5
    beams = R.beam_decode(x, W)
    assert 1 <= len(beams) <= W
    scores = [s for _, _, s in beams]
    assert scores == sorted(scores, reverse=True)
    for l, _, s in beams:
        assert s <= -_nll(x, l) + 1e-9, (l, s, -_nll(x, l))


def _peaked(rng, C, T, margin=20.0):
    path = rng.integers(0, C, size=T)
    x = rng.normal(size=(C, T)) * 0.5
    x[path, np.arange(T)] += margin
    return x, path


@pytest.mark.parametrize("W", [1, 4, 16])
def test_best_beam_on_peaked_input_is_the_labelling_probability(W):
    rng = np.random.default_rng(3)
    x, path = _peaked(rng, 5, 30)
    l, fr, s = R.beam_decode(x, W)[0]
    assert l == R.collapse(path)
    assert abs(s + _nll(x, l)) < 1e-6


def test_frames_are_the_emitting_steps_of_the_peak_path():
    rng = np.random.default_rng(4)
    x, path = _peaked(rng, 5, 25)
    l, fr, _ = R.beam_decode(x, 4)[0]
    want = [t for t in range(25) if path[t] != 0 and (t == 0 or path[t] != path[t - 1])]
    assert list(fr) == want
    gl, gf = R.greedy_decode(x)
    assert tuple(gl) == l and gf == want


def test_input_lengths_and_empty_input():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(4, 9))
    assert R.beam_decode(x, 8, input_length=0) == [((), (), 0.0)]
    assert R.beam_decode(x, 8, input_length=4) == R.beam_decode(x[:, :4], 8)
    assert R.greedy_decode(x, input_length=4) == R.greedy_decode(x[:, :4])
    lab, frm, lens, sc = R.beam_decode_batch(np.stack([x, x]), 3, input_lengths=[9, 0])
    assert lens[1].tolist() == [0, 0, 0] and sc[1, 0] == 0.0 and np.isneginf(sc[1, 1:]).all()


def test_fewer_prefixes_than_beams_leave_empty_slots():
    p = np.array([[[0.5], [0.5], [0.0]]])                        # T = 1: labellings (), (1,); class 2 impossible
    lab, frm, lens, sc = R.beam_decode_batch(p, 5, kind="probs")
    assert lens[0].tolist() == [0, 1, 0, 0, 0]                   # () and (1,) tie at log 0.5: the stay's key (0, 0) wins
    assert np.isneginf(sc[0, 2:]).all() and abs(sc[0, 0] - np.log(0.5)) < 1e-12


def test_greedy_is_argmax_then_collapse_with_ties_to_the_lowest_class():
    rng = np.random.default_rng(6)
    x = rng.normal(size=(5, 200))
    x[:, 10] = 0.0
    x[2, 10] = x[3, 10] = 1.0                                    # tie between classes 2 and 3 at frame 10
    x[:, 11] = 0.0
    x[0, 11] = x[4, 11] = 2.0                                    # tie between the blank and class 4
    am = torch.argmax(torch.tensor(x), dim=0).tolist()
    assert am[10] == 2 and am[11] == 0
    want = [a for i, a in enumerate(am) if a != 0 and (i == 0 or a != am[i - 1])]
    labels, frames = R.greedy_decode(x)
    assert labels == want
    assert [am[f] for f in frames] == labels


def test_beam_ties_follow_the_candidate_key():
    # one frame of uniform probabilities: (), (1,) and (2,) score the same; equal scores go to the smaller candidate key
    x = np.zeros((3, 1))
    beams = R.beam_decode(x, 8)
    assert [b[0] for b in beams] == [(), (1,), (2,)]


# ---- host side of wavenet_speech_amd.decoding (no GPU needed: every check runs before a launch)

def test_decoding_refuses_cpu_tensors_and_bad_arguments():
    from wavenet_speech_amd import decoding as D
    x = torch.zeros(2, 5, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.ctc_greedy_decode(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.ctc_beam_decode(x, 4)
    for w in (0, 65):
        with pytest.raises(ValueError, match="beam_width"):
            D.ctc_beam_decode(x, w)
    with pytest.raises(ValueError, match="input"):
        D.ctc_beam_decode(x, 4, input="softmax")
    with pytest.raises(ValueError, match="beam_width"):
        D.CTCBeamDecoder(" AGCT", beam_width=65)


def test_label_strings():
    from wavenet_speech_amd import labels_to_strings
    from wavenet_speech_amd.modules import sequence_decoders as S
    lab = torch.tensor([[1, 2, 3, 4, 0, 0], [4, 4, 1, 0, 0, 0]], dtype=torch.int32)
    assert labels_to_strings(lab, torch.tensor([4, 3])) == ["AGCT", "TTA"]
    assert labels_to_strings(lab[:, :3]) == ["AGC", "TTA"]
    assert S.labels2strings(torch.tensor([[1, 0, 2, 2, 0, 4]])) == ["AGGT"]  # no collapse: blanks are ''
    logits = torch.randn(2, 7, 5)
    assert torch.equal(S.argmax_decode(logits), logits.max(dim=2)[1])


# ---- the tie-group matcher the GPU decoders are compared through (ctc_decode_ref.match_beams)

def _matcher_fixture():
    """one utterance, W = 8, T = 4: scores with a clear rank 0, a run of three (ranks 1-3), a clear rank 4, a run of two (5-6),
    and rank 7 dead"""
    scores = np.array([[-1.0, -2.0, -2.0005, -2.001, -3.0, -4.0, -4.0008, -np.inf]])
    rows = [(1,), (2, 1), (1, 2), (3,), (1, 1), (2,), (2, 2), ()]
    labels = np.zeros((1, 8, 4), dtype=np.int64)
    lengths = np.zeros((1, 8), dtype=np.int64)
    for w, r in enumerate(rows):
        labels[0, w, :len(r)] = r
        lengths[0, w] = len(r)
    return labels, lengths, scores


def _swap(result, u, v):
    labels, lengths, scores = (a.copy() for a in result)
    labels[0, [u, v]] = labels[0, [v, u]]
    lengths[0, [u, v]] = lengths[0, [v, u]]
    return labels, lengths, scores


def test_tie_runs_split_at_gaps_above_the_threshold():
    assert R.tie_runs(np.array([-1.0, -2.0, -2.0005, -2.001, -3.0, -4.0, -4.0008])) == [(0, 1), (1, 4), (4, 5), (5, 7)]
    assert R.tie_runs(np.array([])) == [] and R.tie_runs(np.array([-5.0])) == [(0, 1)]
    assert R.tie_runs(np.array([-1.0, -1.0 - 1e-3 * 1.01])) == [(0, 1), (1, 2)]


def test_matcher_accepts_the_reference_and_a_swap_inside_a_run():
    want = _matcher_fixture()
    assert R.match_beams(want, want, 4) == 1.0                       # 7 finite ranks of 8: nothing was pruned, no run is open
    assert R.match_beams(want, _swap(want, 1, 3), 4) == 1.0
    assert R.match_beams(want, _swap(want, 5, 6), 4) == 1.0


def test_matcher_leaves_only_the_run_at_the_pruning_edge_unchecked():
    labels, lengths, scores = _matcher_fixture()
    full = (labels[:, :7], lengths[:, :7], scores[:, :7])            # W = 7: every rank finite, the run 5-6 holds the last kept rank
    assert R.match_beams(full, full, 4) == pytest.approx(5 / 7)
    other = tuple(a.copy() for a in full)
    other[0][0, 6, :2] = (3, 1)                                      # another member of the open run: accepted, in range
    assert R.match_beams(full, other, 4) == pytest.approx(5 / 7)
    assert R.match_beams(full, other, 4, next_scores=np.array([-4.0012])) == pytest.approx(5 / 7)   # the pruned one is as close
    with pytest.raises(AssertionError):
        R.match_beams(full, other, 4, next_scores=np.array([-4.5]))  # the pruned candidate is clear of the run: the run is closed
    assert R.match_beams(full, full, 4, next_scores=np.array([-4.5])) == 1.0
    assert R.match_beams(full, full, 4, next_scores=np.array([-np.inf])) == 1.0
    for bad_row, bad_len in (((4, 1), 2), ((0, 1), 2), ((1, 1, 1, 1), 5)):   # label >= classes, the blank, longer than T
        broken = tuple(a.copy() for a in full)
        broken[0][0, 6, :len(bad_row)] = bad_row
        broken[1][0, 6] = bad_len
        with pytest.raises(AssertionError):
            R.match_beams(full, broken, 4)


def test_matcher_rejects_what_is_wrong():
    want = _matcher_fixture()
    one_label = tuple(a.copy() for a in want)
    one_label[0][0, 4, 1] = 2                                        # clear rank 4: (1, 1) -> (1, 2)
    with pytest.raises(AssertionError, match="ranks 4..4"):
        R.match_beams(want, one_label, 4)
    with pytest.raises(AssertionError, match="labellings"):
        R.match_beams(want, _swap(want, 3, 4), 4)                    # across two runs
    with pytest.raises(AssertionError, match="labellings"):
        R.match_beams(want, _swap(want, 0, 1), 4)
    off = tuple(a.copy() for a in want)
    off[2][0, 2] += 1e-2
    with pytest.raises(AssertionError, match="score off"):
        R.match_beams(want, off, 4)
    dead = tuple(a.copy() for a in want)
    dead[2][0, 6] = -np.inf
    with pytest.raises(AssertionError, match="finite ranks"):
        R.match_beams(want, dead, 4)
    alive = tuple(a.copy() for a in want)
    alive[2][0, 7] = -5.0
    with pytest.raises(AssertionError, match="finite ranks"):
        R.match_beams(want, alive, 4)
    nan = tuple(a.copy() for a in want)
    nan[2][0, 7] = np.nan
    with pytest.raises(AssertionError):
        R.match_beams(want, nan, 4)


def test_matcher_scores_are_held_to_the_relative_bound():
    labels, lengths, scores = _matcher_fixture()
    far = (labels, lengths, scores * 1000.0)                         # -1000 ... -4000.8: every rank clear
    near = (labels, lengths, far[2] + 0.09)                          # within 1e-4 |s| + 1e-3 of -1000
    assert R.match_beams(far, near, 4) == 1.0
    with pytest.raises(AssertionError, match="score off"):
        R.match_beams(far, (labels, lengths, far[2] + 0.11), 4)


def test_the_pruned_score_is_the_next_beam_of_a_wider_search():
    rng = np.random.default_rng(11)
    x = rng.normal(size=(4, 3)) * 1.5                                # T = 3: 16 beams prune nothing, so they are the exact order
    wide = R.beam_decode(x, 64)
    beams, pruned = R.beam_decode(x, len(wide), with_next=True)
    assert pruned == -np.inf and beams == wide
    l, f, n, s, nxt = R.beam_decode_batch(x[None], 64, with_next=True)
    assert nxt.tolist() == [-np.inf] and R.beam_decode_batch(x[None], 64)[3].tolist() == s.tolist()
    # one frame: the candidates are (), (1,), (2,), (3,) with scores log y: the first pruned one of W = 2 is the third largest
    y = np.sort(R.log_probs(x[:, :1])[:, 0])[::-1]
    assert R.beam_decode(x[:, :1], 2, with_next=True)[1] == pytest.approx(y[2], abs=1e-12)


# ---- the inputs of tests/test_gpu_decode_edges.py: conditions that the reference alone decides

@pytest.mark.parametrize("name", sorted(K.BEAM_CASES))
def test_edge_cases_leave_few_beams_unchecked(name):
    c = K.beam_case(name)
    want, nxt = c.want()
    share = R.match_beams(want, want, c.C, c.blank, nxt, c.input_lengths)
    assert share >= K.MIN_SHARE, share
    assert np.isfinite(want[2]).any()
    if c.truth is not None and name.startswith("blank"):
        assert tuple(want[0][0, 0, :want[1][0, 0]].tolist()) == c.truth and 0 in c.truth


def test_edge_cases_hold_what_their_tests_rely_on():
    (l, n, s), _ = K.beam_case("limits_peaked").want()
    seen = set(l[0][np.arange(l.shape[2])[None, :] < n[0][:, None]].tolist())
    assert 63 in seen and len(seen) >= 56 and min(seen) >= 1         # labels far above 4 on the kept beams, the top class among them
    (l, n, s), _ = K.beam_case("long_flat").want()
    assert -3400.0 < s[0, 0] < -3200.0
    for kind in ("probs", "log_probs"):
        c = K.beam_case("zeros_%s" % kind)
        (l, n, s), _ = c.want()
        assert np.isneginf(s[3]).all() and (n[3] == 0).all()         # nothing survives the all-zero frame
        assert np.isfinite(s[[0, 1, 4]]).all()
        live = int(np.isfinite(s[2]).sum())
        assert 1 < live < c.W and (n[2, live:] == 0).all()           # fewer live prefixes than beams
        assert (c.x[0, 0] == (0.0 if kind == "probs" else -np.inf)).all()
    c = K.beam_case("ragged")
    assert (np.abs(c.x[0]) >= 30.0).all() and c.input_lengths.tolist() == list(K.RAGGED_LENGTHS)
    a, b = K.beam_case("fixed_point"), K.beam_case("fixed_point_shifted")
    assert np.array_equal(b.x.astype(np.float64) - K.SHIFT, a.x.astype(np.float64))   # the shift is exact in fp32
    a, b = K.beam_case("integers"), K.beam_case("integers_shifted")
    assert np.array_equal(b.x.astype(np.float64) - K.SHIFT, a.x.astype(np.float64)) and np.array_equal(a.x, np.round(a.x))


def test_exact_tie_case_ties_bitwise_and_nowhere_else():
    """classes 2 and 3 share their columns: after every step the only score gaps of at most TIE_GAP are exact zeros, between
    labellings that are each other's 2 <-> 3 swap -- so the order of the tied ranks is the candidate-key rule's alone"""
    c = K.beam_case("exact_ties")
    swap = {1: 1, 2: 3, 3: 2}
    ties = 0
    for b in range(c.B):
        for tb in (1, 2, 3):
            beams, pruned = R.beam_decode(c.x[b], c.W, input_length=tb, with_next=True)
            assert pruned == -np.inf                                 # nothing is pruned
            scores = np.array([s for _, _, s in beams])
            for lo, hi in R.tie_runs(scores):
                assert scores[lo] == scores[hi - 1]                  # a run is an exact tie ...
                group = {beams[w][0] for w in range(lo, hi)}
                assert group == {tuple(swap[v] for v in p) for p in group}    # ... closed under the swap
                ties += hi - lo > 1
    assert ties >= 20


def test_greedy_boundary_case_is_what_it_says():
    x, lens, blank, path = K.greedy_boundaries()
    assert np.array_equal(np.argmax(x, axis=1), path)
    labels, frames, n = R.greedy_decode_batch(x, blank, lens)
    assert labels[0, :n[0]].tolist() == [2, 0, 4, 1] and frames[0, :n[0]].tolist() == [62, 100, 254, 511]
    assert [int(v) for v in n] == [4, 3, 3, 4, 3, 3]
    assert frames[3, :4].tolist() == [62, 100, 250, 256]             # the blank at 255 splits label 1 in two emissions
    assert frames[1, :3].tolist() == [62, 100, 254] and frames[4, :3].tolist() == [62, 100, 250]
