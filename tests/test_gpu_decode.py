"""GPU: the CTC decoders (csrc/wn_decode.hip through wavenet_speech_amd.decoding) against the CPU reference of
tests/ctc_decode_ref.py, exact enumeration, and the project's own CTC loss as an upper bound of every beam's probability."""
import numpy as np
import pytest
import torch

from tests import ctc_decode_ref as R
from tests.gpu_labels import decoding as _D
from tests.gpu_util import DEV, peaked_logits, random_logits as _random_logits

pytestmark = pytest.mark.gpu


def _peaked_logits(seed, B, C, T, margin=5.0):
    return peaked_logits(seed, B, C, T, margin)[0]


def test_greedy_matches_the_reference_bitwise_in_both_layouts():
    D = _D()
    x = _random_logits(0, 8, 5, 4096)
    lens = torch.tensor([4096, 4000, 1, 0, 2500, 4095, 257, 256])
    want_l, want_f, want_n = R.greedy_decode_batch(x.numpy(), input_lengths=lens.numpy())
    xd = x.to(DEV)
    labels, lengths, frames = D.ctc_greedy_decode(xd, input_lengths=lens)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int32 and labels.shape == (8, 4096)
    assert np.array_equal(lengths.cpu().numpy(), want_n)
    assert np.array_equal(labels.cpu().numpy(), want_l)
    assert np.array_equal(frames.cpu().numpy(), want_f)
    xt = xd.transpose(1, 2).contiguous()                              # (B, T, C), read through its strides
    l2, n2, f2 = D.ctc_greedy_decode(xt, input_lengths=lens, layout="BTC")
    assert torch.equal(l2, labels) and torch.equal(n2, lengths) and torch.equal(f2, frames)
    l3, n3, f3 = D.ctc_greedy_decode(xd.transpose(1, 2), input_lengths=lens, layout="BTC")   # a non-contiguous view
    assert torch.equal(l3, labels) and torch.equal(n3, lengths) and torch.equal(f3, frames)


def test_greedy_ties_go_to_the_lowest_class():
    D = _D()
    x = torch.zeros(1, 5, 6)
    x[0, 2, 0] = x[0, 3, 0] = 1.0                                    # tie 2 / 3 -> 2
    x[0, 0, 1] = x[0, 4, 1] = 1.0                                    # tie blank / 4 -> blank
    x[0, 4, 2] = x[0, 1, 2] = 1.0                                    # tie 1 / 4 -> 1
    x[0, 1, 3] = 1.0
    x[0, 3, 4] = 1.0
    labels, lengths, frames = D.ctc_greedy_decode(x.to(DEV))
    assert lengths.tolist() == [3]
    assert labels[0, :3].tolist() == [2, 1, 3] and frames[0, :3].tolist() == [0, 2, 4]   # 1 at frames 2 and 3 collapses


@pytest.mark.parametrize("C,T", [(3, 1), (3, 3), (3, 5), (4, 2), (4, 3)])
def test_beam_against_enumeration(C, T):
    D = _D()
    x = _random_logits(10 * C + T, 4, C, T)
    labels, lengths, scores, frames = D.ctc_beam_decode(x.to(DEV), 64)
    labels, lengths, scores = labels.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()
    for b in range(4):
        exact = sorted(R.exact_labelling_log_probs(x[b].double().numpy()).items(), key=lambda kv: -kv[1])
        got = [tuple(labels[b, w, :lengths[b, w]].tolist()) for w in range(len(exact))]
        assert got == [l for l, _ in exact]
        assert np.abs(scores[b, :len(exact)] - np.array([v for _, v in exact])).max() < 1e-5
        assert np.isneginf(scores[b, len(exact):]).all() and (lengths[b, len(exact):] == 0).all()


def _per_beam_nll(x, labels, lengths):
    """-log p(labelling) of every beam by the project's own CTC loss (training.ctc_total, one utterance per call)"""
    from wavenet_speech_amd import training as TR
    B, W = lengths.shape
    out = np.zeros((B, W))
    for b in range(B):
        for w in range(W):
            n = int(lengths[b, w])
            lab = labels[b:b + 1, w, :max(n, 1)].long()
            out[b, w] = float(TR.ctc_total(x[b:b + 1], lab, torch.tensor([n], device=DEV)))
    return out


def _clear(scores, w):
    """rank w's reference score is more than 1e-3 away from its neighbours' (its labelling is not a near-tie)"""
    W = len(scores)
    gap = min(scores[w - 1] - scores[w] if w > 0 else np.inf, scores[w] - scores[w + 1] if w + 1 < W else np.inf)
    return gap > 1e-3


def _compare_with_reference(x, W, check_nll_beams, check_frames):
    D = _D()
    xd = x.to(DEV)
    labels, lengths, scores, frames = D.ctc_beam_decode(xd, W)
    want_l, want_f, want_n, want_s = R.beam_decode_batch(x.numpy(), W)
    gl, gn, gs, gf = labels.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy().astype(np.float64), frames.cpu().numpy()
    assert np.isfinite(gs).all() and np.isfinite(want_s).all()
    assert (np.abs(gs - want_s) <= 1e-4 * np.abs(want_s) + 1e-3).all(), np.abs(gs - want_s).max()
    assert (np.diff(gs, axis=1) <= 0).all()                           # sorted descending
    B = x.shape[0]
    for b in range(B):
        for w in range(W):
            n = gn[b, w]
            assert (np.diff(gf[b, w, :n]) > 0).all() and (gf[b, w, :n] < x.shape[2]).all()   # frames rise along the prefix
            if _clear(want_s[b], w):
                n = want_n[b, w]
                assert gn[b, w] == n and np.array_equal(gl[b, w, :n], want_l[b, w, :n]), (b, w)
                # backpointers follow ranks at every step, which near-ties deep in the search may swap: frames of the best
                # beam on peaked input only
                if check_frames and w == 0:
                    assert np.array_equal(gf[b, w, :n], want_f[b, w, :n]), (b, w)
    assert (gl[np.arange(gl.shape[-1])[None, None, :] >= gn[:, :, None]] == 0).all()   # zero padding
    nll = _per_beam_nll(xd, labels, lengths[:, :check_nll_beams].contiguous())
    ub = -nll
    assert (gs[:, :check_nll_beams] <= ub + 1e-4 * np.abs(ub) + 1e-3).all()
    return gs, ub


@pytest.mark.parametrize("W", [1, 8, 64])
def test_beam_against_the_reference_on_random_logits(W):
    _compare_with_reference(_random_logits(1 + W, 8, 5, 1000), W, min(W, 4), False)


@pytest.mark.parametrize("W", [1, 8, 64])
def test_beam_against_the_reference_on_peaked_logits(W):
    _compare_with_reference(_peaked_logits(2 + W, 8, 5, 1000), W, min(W, 4), True)


def test_best_beam_on_strongly_peaked_input_is_the_labelling_probability():
    D = _D()
    rng = np.random.default_rng(8)
    B, C, T = 4, 5, 200
    path = rng.integers(0, C, size=(B, T))
    x = rng.normal(size=(B, C, T)) * 0.5
    x[np.arange(B)[:, None], path, np.arange(T)[None, :]] += 20.0     # off-path mass e^-20 per class and frame
    xd = torch.tensor(x, dtype=torch.float32, device=DEV)
    labels, lengths, scores, _ = D.ctc_beam_decode(xd, 8)
    ub = -_per_beam_nll(xd, labels, lengths[:, :1].contiguous())
    for b in range(B):
        assert tuple(labels[b, 0, :int(lengths[b, 0])].tolist()) == R.collapse(path[b])
    assert np.abs(scores[:, 0].cpu().numpy() - ub[:, 0]).max() < 1e-3


def test_input_kinds_give_the_same_beams():
    D = _D()
    x = _random_logits(3, 4, 5, 300).to(DEV)
    lp = torch.log_softmax(x, dim=1)
    a = D.ctc_beam_decode(x, 8, input="logits")
    b = D.ctc_beam_decode(lp.exp(), 8, input="probs")
    c = D.ctc_beam_decode(lp, 8, input="log_probs")
    sa = a[2].cpu().numpy().astype(np.float64)
    for other in (b, c):
        assert torch.allclose(other[2], a[2], rtol=1e-5, atol=1e-3)
        for i in range(4):
            for w in range(8):
                if _clear(sa[i], w):                             # fp32 rounding differs between the forms: near-ties may swap
                    n = int(a[1][i, w])
                    assert int(other[1][i, w]) == n and torch.equal(other[0][i, w, :n], a[0][i, w, :n])
    d = D.ctc_beam_decode(lp.exp().transpose(1, 2), 8, input="probs", layout="BTC")
    assert torch.equal(d[0], b[0]) and torch.equal(d[2], b[2]) and torch.equal(d[3], b[3])


def test_two_runs_are_bitwise_identical():
    D = _D()
    x = _random_logits(4, 8, 5, 1000).to(DEV)
    lens = torch.tensor([1000, 999, 500, 0, 1, 64, 700, 1000])
    r1 = D.ctc_beam_decode(x, 16, input_lengths=lens)
    r2 = D.ctc_beam_decode(x, 16, input_lengths=lens)
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    assert r1[1][3].tolist() == [0] * 16 and float(r1[2][3, 0]) == 0.0 and torch.isinf(r1[2][3, 1:]).all()


def test_recovers_a_known_read():
    D = _D()
    from wavenet_speech_amd import labels_to_strings
    rng = np.random.default_rng(5)
    read = rng.integers(1, 5, size=60)
    cols = []
    for i, base in enumerate(read):
        if i > 0 and read[i - 1] == base:
            cols += [0] * int(rng.integers(1, 3))                    # a repeated base needs a blank in between
        cols += [int(base)] * int(rng.integers(3, 9))                # upsampled: several frames per base
        cols += [0] * int(rng.integers(0, 3))
    T = len(cols)
    x = rng.normal(size=(1, 5, T)) * 0.5
    x[0, cols, np.arange(T)] += 5.0
    xd = torch.tensor(x, dtype=torch.float32, device=DEV)
    want = "".join(" AGCT"[v] for v in read)
    gl, gn, _ = D.ctc_greedy_decode(xd)
    assert labels_to_strings(gl, gn) == [want]
    bl, bn, bs, _ = D.ctc_beam_decode(xd, 8)
    assert labels_to_strings(bl[:, 0], bn[:, 0]) == [want]
    assert bl[0, 0, :len(read)].cpu().tolist() == read.tolist()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_end_to_end_from_a_raw_ctcnet(precision):
    D = _D()
    import wavenet_speech_amd as W
    from wavenet_speech_amd.modules.raw_ctcnet import RawCTCNet
    torch.manual_seed(0)
    rl = [(64, 64, 2, d) for d in (1, 2, 4)]
    net = RawCTCNet(64, 3, 5, rl, 64, softmax=False, causal=False).to(DEV)
    if precision != "f32":
        W.set_precision(net, precision)
    sig = torch.randn(2, 1, 400, device=DEV)
    with torch.no_grad():
        logits = net(sig)
    assert logits.shape[:2] == (2, 5)
    labels, lengths, scores, frames = D.ctc_beam_decode(logits, 8)
    want_l, want_f, want_n, want_s = R.beam_decode_batch(logits.float().cpu().numpy(), 8)
    gs = scores.cpu().numpy().astype(np.float64)
    assert (np.abs(gs - want_s) <= 1e-4 * np.abs(want_s) + 1e-3).all()
    for b in range(2):
        for w in range(8):
            if _clear(want_s[b], w):
                n = want_n[b, w]
                assert lengths[b, w].item() == n and labels[b, w, :n].cpu().tolist() == want_l[b, w, :n].tolist()
    gl, gn, gf = D.ctc_greedy_decode(logits)
    rl_, rf_, rn_ = R.greedy_decode_batch(logits.float().cpu().numpy())
    assert np.array_equal(gn.cpu().numpy(), rn_) and np.array_equal(gl.cpu().numpy(), rl_)


def test_bad_input_is_reported_through_the_device_flag():
    D = _D()
    import wavenet_speech_amd as W
    W.check_device_flags()
    x = _random_logits(6, 3, 5, 50).to(DEV)
    labels, lengths, scores, _ = D.ctc_beam_decode(x, 4, input_lengths=torch.tensor([50, 51, -1]))
    with pytest.raises(RuntimeError, match="2 utterance"):
        W.check_device_flags()
    assert lengths[1:].abs().sum().item() == 0 and torch.isnan(scores[1:]).all() and torch.isfinite(scores[0, 0])
    D.ctc_greedy_decode(x, input_lengths=torch.tensor([50, 60, 10]))
    with pytest.raises(RuntimeError, match="1 utterance"):
        W.check_device_flags()
    D.ctc_beam_decode(x, 4, blank=5)
    with pytest.raises(RuntimeError, match="blank"):
        W.check_device_flags()
    D.ctc_greedy_decode(x, blank=-1)
    with pytest.raises(RuntimeError, match="3 utterance"):
        W.check_device_flags()


def test_limits_raise_before_launch():
    D = _D()
    x = torch.zeros(2, 5, 10, device=DEV)
    for w in (0, 65):
        with pytest.raises(ValueError, match="beam_width"):
            D.ctc_beam_decode(x, w)
    big = torch.zeros(2, 65, 10, device=DEV)
    with pytest.raises(ValueError, match="classes"):
        D.ctc_beam_decode(big, 4)
    with pytest.raises(ValueError, match="classes"):
        D.ctc_greedy_decode(big)
    with pytest.raises(ValueError, match="input_lengths"):
        D.ctc_beam_decode(x, 4, input_lengths=torch.tensor([1, 2, 3]))


def test_ctcdecode_calling_shape():
    D = _D()
    x = _random_logits(7, 2, 5, 120).to(DEV)
    probs = torch.softmax(x, dim=1).transpose(1, 2).contiguous()     # (B, T, C), as the notebook hands it to ctcdecode
    dec = D.CTCBeamDecoder(["_", "A", "G", "C", "T"], beam_width=7, blank_id=0)
    beam_results, beam_scores, timesteps, out_lens = dec.decode(probs)
    assert beam_results.shape == (2, 7, 120) and beam_scores.shape == (2, 7) and out_lens.shape == (2, 7)
    l, n, s, f = D.ctc_beam_decode(probs.transpose(1, 2), 7, input="probs")
    assert torch.equal(beam_results, l) and torch.equal(out_lens, n) and torch.equal(timesteps, f) and torch.equal(beam_scores, s)
    lp = D.CTCBeamDecoder(" AGCT", beam_width=7, log_probs_input=True).decode(torch.log(probs), seq_lens=torch.tensor([120, 60]))
    assert lp[0].shape == (2, 7, 120) and int(lp[3][1].max()) <= 60
