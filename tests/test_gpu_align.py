"""GPU: CTC forced alignment (csrc/wn_align.hip through wavenet_speech_amd.ctc_forced_align) against the float64 CPU reference
of tests/ctc_align_ref.py, exhaustive enumeration, the project's own CTC loss (an upper bound of every alignment's probability)
and the greedy decoder.

The margin rule.  Where two alignments score within rounding of each other the device and the reference may legitimately pick
different ones, so states are compared at every frame whose reference MARGIN (optimum minus the best path that avoids the
reference's state at that frame, ctc_align_ref.frame_margins) exceeds 1e-6; different evaluation orders of the fp64 reference
disagree by no more than 3e-11 in score, four orders of magnitude below that.  At most 0.1 % of an utterance's frames may be
excluded this way (a condition, not a measurement), and the device's whole path, re-scored on the host under the reference's
fp64 log-probabilities, must be within 1e-9 |score| of the reference optimum -- so a different path is an equally good one.
The exact test uses log-probabilities on a quarter grid, where every sum is exact and ties are real: bit-identical, ties
included."""
import numpy as np
import pytest
import torch

from tests import ctc_align_ref as A
from tests.gpu_labels import check_forced_batch as _check_batch, check_utterance as _check_utterance, forced_align as _run, package as _W
from tests.gpu_labels import pad_targets as _pad
from tests.gpu_util import DEV, peaked_logits as _peaked_logits, random_logits as _random_logits

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ 1. exact, with ties

def test_exact_on_a_quarter_grid_ties_included():
    rng = np.random.default_rng(7)
    B, C, T = 6, 5, 512
    x = torch.tensor(rng.integers(-24, 1, size=(B, C, T)) / 4.0, dtype=torch.float32)
    lens = [90, 90, 37, 1, 0, 60]
    label_lists = [rng.integers(1, C, size=n).tolist() for n in lens]
    label_lists[5] = np.repeat(rng.integers(1, C, size=30), 2).tolist()      # every second label repeats: 30 forced blanks
    in_len = torch.tensor([512, 300, 512, 7, 512, 181])
    # the reference itself must meet exact ties, or the tie rule is not exercised
    lp0 = x[0].double().numpy()
    ref_states, _, _ = A.viterbi_align(lp0, label_lists[0])
    tied = int((A.frame_margins(lp0, label_lists[0], ref_states) == 0).sum())
    print("tied frames in utterance 0:", tied)
    assert tied >= 1
    got = _run(x, label_lists, in_len, input="log_probs")
    _check_batch(x, label_lists, in_len, got, kind="log_probs", exact=True, tag="grid")


# ---------------------------------------------------------------------------------------------------- 2. full-size fp32 logits

FULL_LENGTHS = [4096, 4000, 3500, 4096, 2500, 4095, 3000, 4096]


@pytest.mark.parametrize("seed", [0, 1])
def test_full_size_random_logits(seed):
    B, C, T = 8, 5, 4096
    x = _random_logits(20 + seed, B, C, T)
    rng = np.random.default_rng(30 + seed)
    label_lists = [rng.integers(1, C, size=600).tolist() for _ in range(B)]
    in_len = torch.tensor(FULL_LENGTHS)
    got = _run(x, label_lists, in_len)
    _check_batch(x, label_lists, in_len, got, tag="random")


@pytest.mark.parametrize("seed", [0, 1])
def test_full_size_peaked_logits(seed):
    B, C, T = 8, 5, 4096
    x, path = _peaked_logits(40 + seed, B, C, T)
    label_lists = [A.collapse(path[b, :FULL_LENGTHS[b]]) for b in range(B)]
    # a whole utterance: 4096 / 3 runs, 4 in 5 not blank, 4 in 5 of those not merged into an equal neighbour -- about 870 labels
    assert 780 <= len(label_lists[0]) <= 960, len(label_lists[0])
    in_len = torch.tensor(FULL_LENGTHS)
    got = _run(x, label_lists, in_len)
    _check_batch(x, label_lists, in_len, got, tag="peaked")


# ------------------------------------------------------------------------------------------------------------------ 3. enumeration

@pytest.mark.parametrize("C,T,L", [(3, 1, 0), (3, 1, 1), (3, 2, 2), (3, 3, 1), (3, 5, 2), (3, 6, 3), (3, 6, 2), (4, 4, 2), (4, 5, 1),
                                   (4, 5, 3), (3, 4, 0)])
def test_against_enumeration(C, T, L):
    B = 4
    x = _random_logits(100 * C + 10 * T + L, B, C, T)
    rng = np.random.default_rng(1000 * C + 10 * T + L)
    label_lists = [rng.integers(1, C, size=L).tolist() for _ in range(B)]
    states, frame_labels, spans, score = _run(x, label_lists)
    for b in range(B):
        lp = A.log_softmax(x[b].double().numpy())
        want = A.best_score_by_enumeration(lp, label_lists[b])
        if np.isneginf(want):
            assert np.isneginf(score[b]) and (states[b] == -1).all() and (frame_labels[b] == -1).all() and (spans[b] == -1).all()
            continue
        assert abs(float(score[b]) - want) <= 1e-6 * abs(want)
        assert abs(A.path_score(lp, label_lists[b], states[b]) - want) <= 1e-9 * abs(want)
        assert A.collapse(frame_labels[b]) == label_lists[b]
    _check_batch(x, label_lists, None, (states, frame_labels, spans, score), tag="enum")


# ------------------------------------------------------------------------------------------------- 4. bound by the project's loss

def _nll(x, labels):
    from wavenet_speech_amd import training as TR
    lab = torch.tensor([labels if labels else [1]], device=DEV)
    return float(TR.ctc_total(x.to(DEV), lab, torch.tensor([len(labels)], device=DEV)))


def test_score_is_bounded_by_the_ctc_loss():
    B, C, T = 4, 5, 600
    x = _random_logits(50, B, C, T)
    rng = np.random.default_rng(51)
    label_lists = [rng.integers(1, C, size=n).tolist() for n in (80, 150, 1, 0)]
    in_len = [600, 420, 600, 333]
    states, frame_labels, spans, score = _run(x, label_lists, torch.tensor(in_len))
    for b in range(B):
        nll = _nll(x[b:b + 1, :, :in_len[b]].contiguous(), label_lists[b])
        print("utterance %d: score %.6f, -nll %.6f" % (b, score[b], -nll))
        assert np.isfinite(nll) and float(score[b]) <= -nll + 1e-5 * abs(nll)


def test_a_single_alignment_equals_the_loss():
    """T_b = L_b without repeats: exactly one alignment (every frame its label, no blank), so the best path IS the sum"""
    C, L = 5, 300
    rng = np.random.default_rng(52)
    labels = [1]
    while len(labels) < L:
        v = int(rng.integers(1, C))
        if v != labels[-1]:
            labels.append(v)
    x = _random_logits(53, 1, C, L)
    states, frame_labels, spans, score = _run(x, [labels])
    assert states[0].tolist() == list(range(1, 2 * L, 2)) and frame_labels[0].tolist() == labels
    assert spans[0].tolist() == [[j, j + 1] for j in range(L)]
    nll = _nll(x, labels)
    print("single alignment: score %.6f, -nll %.6f" % (score[0], -nll))
    assert abs(float(score[0]) + nll) <= 2e-6 * abs(nll)


# -------------------------------------------------------------------------------------------------- 5. the greedy decoder's path

def test_aligning_the_greedy_labels_gives_the_argmax_path():
    W = _W()
    B, C, T = 4, 5, 1000
    x, _ = _peaked_logits(60, B, C, T)
    xd = x.to(DEV)
    in_len = torch.tensor([1000, 999, 640, 65])
    targets, lengths, frames = W.ctc_greedy_decode(xd, input_lengths=in_len)
    lmax = int(lengths.max())
    out = W.ctc_forced_align(xd, targets[:, :lmax], lengths, input_lengths=in_len)
    torch.cuda.synchronize()
    argmax = xd.argmax(dim=1).to(torch.int32)
    for b in range(B):
        n, tb = int(lengths[b]), int(in_len[b])
        assert torch.equal(out.frame_labels[b, :tb], argmax[b, :tb])             # the argmax path is the global optimum
        assert (out.frame_labels[b, tb:] == -1).all()
        assert torch.equal(out.spans[b, :n, 0], frames[b, :n])                   # a label starts where greedy emitted it
        assert A.collapse(out.frame_labels[b, :tb].cpu().numpy()) == targets[b, :n].cpu().tolist()
        want = torch.log_softmax(x[b, :, :tb].double(), dim=0).max(dim=0).values.sum().item()
        assert abs(float(out.score[b]) - want) <= 1e-6 * abs(want)


# ----------------------------------------------------------------------------------------------------- 6. layouts and input kinds

def test_layouts_give_the_same_result():
    W = _W()
    B, C, T = 3, 5, 300
    x = _random_logits(70, B, C, T).to(DEV)
    rng = np.random.default_rng(71)
    targets, tlens = _pad([rng.integers(1, C, size=n).tolist() for n in (40, 25, 60)])
    in_len = torch.tensor([300, 211, 300])
    a = W.ctc_forced_align(x, targets, tlens, input_lengths=in_len)
    b = W.ctc_forced_align(x.transpose(1, 2).contiguous(), targets, tlens, input_lengths=in_len, layout="BTC")
    btc = x.transpose(1, 2).contiguous()
    c = W.ctc_forced_align(btc.transpose(1, 2), targets, tlens, input_lengths=in_len, layout="BCT")   # a non-contiguous view
    d = W.ctc_forced_align(x.transpose(1, 2), targets, tlens, input_lengths=in_len, layout="BTC")     # a non-contiguous view
    for other in (b, c, d):
        for u, v in zip(a, other):
            assert torch.equal(u, v)
    assert torch.isfinite(a.score).all()


@pytest.mark.parametrize("kind", ["logits", "probs", "log_probs"])
def test_input_kinds_match_the_reference(kind):
    B, C, T = 3, 5, 400
    x = _random_logits(72, B, C, T)
    if kind == "probs":
        x = torch.softmax(x, dim=1)
        x[1, 2, 17] = 0.0                                            # a probability of 0: log-probability -inf, never on the path
    elif kind == "log_probs":
        x = torch.log_softmax(x, dim=1)
    rng = np.random.default_rng(73)
    label_lists = [rng.integers(1, C, size=n).tolist() for n in (50, 33, 120)]
    in_len = torch.tensor([400, 400, 377])
    got = _run(x, label_lists, in_len, input=kind)
    _check_batch(x, label_lists, in_len, got, kind=kind, tag=kind)


# ---------------------------------------------------------------------------------------------------------------- 7. edge cases

def test_edge_cases_and_poisoned_rows():
    W = _W()
    W.check_device_flags()
    C, T, Lmax = 5, 20, 6
    rows = [
        ([1, 2, 3], 20),                   # 0 ordinary
        ([1, 1, 1, 1, 1, 1], 8),           # 1 infeasible: 6 labels + 5 repeats > 8 frames
        ([], 0),                           # 2 no frames, no labels: score 0
        ([2, 3], 0),                       # 3 no frames but labels: -inf
        ([], 20),                          # 4 no labels: all blank
        ([1, 0, 2], 20),                   # 5 poisoned: a label equal to the blank
        ([1, 5, 2], 20),                   # 6 poisoned: a label >= C
        ([1, -2, 2], 20),                  # 7 poisoned: a negative label
        ([4, 4, 2, 1], 20),                # 8 ordinary, between poisoned rows
        ([1, 2], 20),                      # 9 poisoned below: label_length > Lmax
        ([1, 2], 21),                      # 10 poisoned: input_length > T
        ([3, 1, 2, 2], 6),                 # 11 ordinary, one frame to spare: 4 labels + 1 repeat in 6 frames
    ]
    B = len(rows)
    x = _random_logits(80, B, C, T)
    label_lists = [r[0] for r in rows]
    targets, tlens = _pad(label_lists, Lmax)
    tlens[9] = Lmax + 1
    in_len = torch.tensor([r[1] for r in rows])
    out = W.ctc_forced_align(x.to(DEV), targets, tlens, input_lengths=in_len)
    with pytest.raises(RuntimeError, match="5 utterance"):
        W.check_device_flags()
    states, frame_labels, spans, score = [v.cpu().numpy() for v in out]
    good = [0, 1, 2, 3, 4, 8, 11]
    for b in good:
        lp = A.log_softmax(x[b].double().numpy()[:, :rows[b][1]])
        _check_utterance(lp, label_lists[b], states[b], frame_labels[b], spans[b], score[b], tag="edge[%d]" % b)
    assert np.isneginf(score[1]) and (states[1] == -1).all() and (spans[1] == -1).all()
    assert score[2] == 0.0 and (states[2] == -1).all()
    assert np.isneginf(score[3]) and (states[3] == -1).all() and (spans[3] == -1).all()
    assert (states[4] == 0).all() and (frame_labels[4] == 0).all() and (spans[4] == -1).all() and np.isfinite(score[4])
    for b in (5, 6, 7, 9, 10):
        assert np.isnan(score[b]) and (states[b] == -1).all() and (frame_labels[b] == -1).all() and (spans[b] == -1).all(), b
    # the poisoned rows do not disturb their neighbours: the same rows alone give the same bits
    keep = torch.tensor(good)
    alone = W.ctc_forced_align(x[keep].to(DEV), targets[keep], tlens[keep], input_lengths=in_len[keep])
    W.check_device_flags()
    for u, v in zip(out, alone):
        assert torch.equal(u[keep.to(DEV)], v)
    # a blank other than 0, and frame labels / spans left out at the C ABI are covered by the Python surface's own checks
    alt = W.ctc_forced_align(x[:1].to(DEV), torch.tensor([[0, 1, 3]]), torch.tensor([3]), blank=4)
    s4, f4, p4, sc4 = [v.cpu().numpy() for v in alt]
    lp = A.log_softmax(x[0].double().numpy())
    want_states, want_score, want_spans = A.viterbi_align(lp, [0, 1, 3], blank=4)
    assert abs(float(sc4[0]) - want_score) <= 1e-6 * abs(want_score)
    assert np.array_equal(f4[0], A.frame_labels_of(s4[0], [0, 1, 3], blank=4))
    assert abs(A.path_score(lp, [0, 1, 3], s4[0], blank=4) - want_score) <= 1e-9 * abs(want_score)
    W.check_device_flags()


def test_cpu_tensors_and_bad_arguments_raise():
    W = _W()
    x = torch.zeros(2, 5, 10)
    t, n = torch.tensor([[1, 2], [3, 4]]), torch.tensor([2, 2])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        W.ctc_forced_align(x, t, n)
    xd = x.to(DEV)
    with pytest.raises(ValueError, match="input must be"):
        W.ctc_forced_align(xd, t, n, input="softmax")
    with pytest.raises(ValueError, match="targets"):
        W.ctc_forced_align(xd, t.float(), n)
    with pytest.raises(ValueError, match="targets"):
        W.ctc_forced_align(xd, t[:1], n)
    with pytest.raises(ValueError, match="target_lengths"):
        W.ctc_forced_align(xd, t, torch.tensor([2]))
    with pytest.raises(ValueError, match="blank"):
        W.ctc_forced_align(xd, t, n, blank=5)
    with pytest.raises(ValueError, match="at most 2047"):
        W.ctc_forced_align(xd, torch.ones(2, 2048, dtype=torch.long), n)
    with pytest.raises(ValueError, match="classes"):
        W.ctc_forced_align(torch.zeros(2, 65, 10, device=DEV), t, n)
    out = W.ctc_forced_align(xd, torch.zeros(2, 0, dtype=torch.int16), torch.tensor([0, 0]))    # no label columns at all
    assert out.spans.shape == (2, 0, 2) and (out.states == 0).all() and torch.isfinite(out.score).all()
    out = W.ctc_forced_align(xd, t.to(torch.int32), n.to(torch.int16))                          # any integer dtype
    assert torch.isfinite(out.score).all()
    W.check_device_flags()


# ---------------------------------------------------------------------------------------------------------------- 8. limit shape

def test_the_limit_shape_2047_labels():
    C, T, L = 5, 4200, 2047
    x = _random_logits(90, 2, C, T)
    rng = np.random.default_rng(91)
    label_lists = [rng.integers(1, C, size=L).tolist(), rng.integers(1, C, size=5).tolist()]
    in_len = torch.tensor([4200, 50])
    got = _run(x, label_lists, in_len)
    _check_batch(x, label_lists, in_len, got, tag="limit")
    assert np.isfinite(got[3]).all()


def test_several_waves_between_the_sizes():
    """label counts around the thread-count steps (one wave up to 255 labels, then one more wave per 256 labels)"""
    C, T = 5, 1500
    for L in (255, 256, 300, 511, 512, 1023):
        x = _random_logits(900 + L, 2, C, T)
        rng = np.random.default_rng(L)
        label_lists = [rng.integers(1, C, size=L).tolist(), rng.integers(1, C, size=L // 3).tolist()]
        in_len = torch.tensor([1500, 1200])
        got = _run(x, label_lists, in_len)
        _check_batch(x, label_lists, in_len, got, tag="L%d" % L)


# ---------------------------------------------------------------------------------------------------------------- 9. determinism

def test_two_runs_are_bitwise_identical_and_the_input_is_untouched():
    W = _W()
    B, C, T = 8, 5, 2000
    x = _random_logits(95, B, C, T).to(DEV)
    keep = x.clone()
    rng = np.random.default_rng(96)
    targets, tlens = _pad([rng.integers(1, C, size=n).tolist() for n in (300, 200, 100, 0, 1, 64, 650, 400)])
    in_len = torch.tensor([2000, 1999, 500, 100, 1, 640, 2000, 1000])
    r1 = W.ctc_forced_align(x, targets, tlens, input_lengths=in_len)
    r2 = W.ctc_forced_align(x, targets, tlens, input_lengths=in_len)
    torch.cuda.synchronize()
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    assert torch.equal(x, keep)
    assert torch.isfinite(r1.score).all()
    W.check_device_flags()
