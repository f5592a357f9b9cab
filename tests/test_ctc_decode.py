"""CPU: the plain-Python CTC decoders of tests/ctc_decode_ref.py (the reference the GPU decoders are held to, test_gpu_decode.py)
against ground truth -- exact enumeration of every alignment, the CTC loss oracle as an upper bound, argmax + collapse -- and the
host-side pieces of wavenet_speech_amd.decoding (argument checks, string helpers) that run without a GPU."""
import numpy as np
import pytest
import torch

from oracle import ctc_oracle as CO
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
