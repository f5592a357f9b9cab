"""GPU: the CTC decoders (csrc/wn_decode.hip) at the edges of what they accept -- 64 classes x 64 beams, two classes, beam widths
that 4 does not divide, any blank, ragged lengths around the 32-frame staging chunk, zeros in the probabilities, exact ties, scores
far from 0, batches and strided views -- against the float64 reference of tests/ctc_decode_ref.py.  Every beam result goes through
ctc_decode_ref.match_beams, which compares near-tied ranks as sets instead of leaving them out; the inputs come from
tests/ctc_decode_cases.py, where tests/test_ctc_decode.py holds the reference alone to a checked share of at least 0.90 per case.
The greedy decoder is compared bitwise.  NaN input is unspecified and not tested."""
import numpy as np
import pytest
import torch

from tests import ctc_decode_cases as K
from tests import ctc_decode_ref as R
from tests.gpu_labels import decoding as _D
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


def _no_flag():
    import wavenet_speech_amd as W
    W.check_device_flags()


def _beam(x, W, blank=0, input_lengths=None, kind="logits", layout="BCT"):
    """-> (labels, lengths, scores, frames) as numpy arrays, scores in float64"""
    x = torch.as_tensor(x)
    lens = None if input_lengths is None else torch.as_tensor(np.asarray(input_lengths))
    labels, lengths, scores, frames = _D().ctc_beam_decode(x.to(DEV), W, blank=blank, input_lengths=lens, input=kind, layout=layout)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int32 and frames.dtype == torch.int32 and lengths.dtype == torch.int32 and scores.dtype == torch.float32
    return labels.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy().astype(np.float64), frames.cpu().numpy()


def _check_structure(got, C, blank, input_lengths):
    """what holds for every result: scores descending, labels in [0, C) and never the blank, frames inside the utterance and
    strictly rising, labels and frames zero at and past lengths[b, w]"""
    gl, gn, gs, gf = got
    B, W, T = gl.shape
    assert not np.isnan(gs).any()
    with np.errstate(invalid="ignore"):
        assert (np.diff(gs, axis=1)[np.isfinite(gs[:, 1:])] <= 0).all()
    valid = np.arange(T)[None, None, :] < gn[:, :, None]
    assert (gn >= 0).all() and (gl[~valid] == 0).all() and (gf[~valid] == 0).all()
    assert ((gl[valid] >= 0) & (gl[valid] < C) & (gl[valid] != blank)).all()
    tb = np.full(B, T) if input_lengths is None else np.asarray(input_lengths)
    assert (gn <= tb[:, None]).all()
    assert ((gf >= 0) & (gf < np.maximum(tb, 1)[:, None, None]))[valid].all()
    rising = np.diff(gf, axis=2) > 0
    assert rising[valid[:, :, 1:]].all()


def _check_case(c, layout="BCT"):
    x = torch.from_numpy(c.x)
    if layout == "BTC":
        x = x.transpose(1, 2).contiguous()
    got = _beam(x, c.W, c.blank, c.input_lengths, c.kind, layout)
    want, nxt = c.want()
    share = R.match_beams(want, got[:3], c.C, c.blank, nxt, c.input_lengths)
    assert share >= K.MIN_SHARE, share
    _check_structure(got, c.C, c.blank, c.input_lengths)
    return got


# ---------------------------------------------------------------------------------------------------------------------- beam

@pytest.mark.parametrize("name", ["limits_peaked", "limits_random"])
def test_beam_at_64_classes_and_64_beams(name):
    """4096 candidates, 90 KB of LDS, 16 rank passes per thread, candidate keys up to 63 * 65 + 64, labels up to 63 in a node"""
    c = K.beam_case(name)
    gl, gn, gs, gf = _check_case(c)
    assert np.isfinite(gs).all()
    if name == "limits_peaked":
        valid = np.arange(c.T)[None, :] < gn[0][:, None]
        seen = set(gl[0][valid].tolist())
        assert 63 in seen and len(seen) >= 56                        # labels far above 4 on the kept beams, the top class among them
    _no_flag()


def test_beam_with_two_classes():
    """the only extension of a non-empty prefix repeats its last label"""
    c = K.beam_case("two_classes")
    gl, gn, gs, gf = _check_case(c)
    assert set(gl.reshape(-1).tolist()) == {0, 1}


@pytest.mark.parametrize("W,C", K.ODD_WIDTHS)
def test_beam_at_widths_that_four_does_not_divide(W, C):
    """the merge search strides the beams by 4 lanes; W x C is no multiple of 64 or 256"""
    assert (W * C) % 64 != 0
    _check_case(K.beam_case("odd_W%d_C%d" % (W, C)))


@pytest.mark.parametrize("blank,kind", K.OTHER_BLANKS)
def test_beam_with_another_blank(blank, kind):
    c = K.beam_case("blank%d_%s" % (blank, kind))
    gl, gn, gs, gf = _check_case(c)
    n = int(gn[0, 0])
    assert tuple(gl[0, 0, :n].tolist()) == c.truth                   # utterance 0: the labelling its peaks spell
    assert n == len(c.truth) and (gl[0, 0, :n] == 0).any() and (gl[0, 0, n:] == 0).all()   # class 0 is a label; `lengths` tells it from padding
    want_l, want_f, want_n, _, _ = c.ref()
    assert np.array_equal(gf[0, 0, :n], want_f[0, 0, :n])            # strongly peaked: the backpointer path is the reference's
    _no_flag()


@pytest.mark.parametrize("layout", ["BCT", "BTC"])
def test_beam_on_ragged_lengths_around_the_staging_chunk(layout):
    """lengths 0, 1, 31 ... 97, 100 of 100 frames, garbage of magnitude 30-60 past each: a frame read past its utterance, or one
    left out, ends on other prefixes and scores"""
    c = K.beam_case("ragged")
    gl, gn, gs, gf = _check_case(c, layout)
    assert gn[0].tolist() == [0] * c.W and gs[0, 0] == 0.0 and np.isneginf(gs[0, 1:]).all()   # length 0: the empty prefix alone
    assert np.isfinite(gs[1]).sum() == c.C                           # length 1: () and the C - 1 single labels, nothing else
    _no_flag()


@pytest.mark.parametrize("kind", ["probs", "log_probs"])
def test_beam_with_zeros_in_the_probabilities(kind):
    """exact zeros (-inf as log_probs): the blank in every frame, a class over 20 frames, one-hot frames that leave fewer live
    prefixes than beams, and an all-zero frame that nothing survives -- without a flag, and without touching the others"""
    _no_flag()
    c = K.beam_case("zeros_%s" % kind)
    gl, gn, gs, gf = _check_case(c)
    assert np.isneginf(gs[3]).all() and (gn[3] == 0).all() and (gl[3] == 0).all() and (gf[3] == 0).all()
    live = int(np.isfinite(gs[2]).sum())
    assert 1 < live < c.W and np.isneginf(gs[2, live:]).all() and (gn[2, live:] == 0).all()
    assert np.isfinite(gs[[0, 1, 4]]).all()
    _no_flag()
    alone = _beam(c.x[4:5], c.W, kind=c.kind)                        # utterance 3 is utterance 4 with one frame zeroed
    for u, v in zip(alone, (gl, gn, gs, gf)):
        assert np.array_equal(u[0], v[4])


def test_beam_orders_exact_ties_by_the_candidate_key():
    """identical columns for classes 2 and 3, nothing pruned: swapped prefixes tie bitwise in any precision, every other gap
    exceeds 1e-3 (tests/test_ctc_decode.py), so every rank must hold the reference's labelling"""
    c = K.beam_case("exact_ties")
    gl, gn, gs, gf = _check_case(c)
    want_l, want_f, want_n, want_s, _ = c.ref()
    assert np.array_equal(gn, want_n) and np.array_equal(gl, want_l)
    assert np.array_equal(gf, want_f)
    tied = 0
    for b in range(c.B):
        for lo, hi in R.tie_runs(want_s[b][np.isfinite(want_s[b])]):
            assert (gs[b, lo:hi] == gs[b, lo]).all()                 # and the ties are exact on the device too
            tied += hi - lo > 1
    assert tied >= 20


ENUM_SHAPES = [(3, 3), (3, 5), (4, 3)]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("C,T", ENUM_SHAPES)
def test_beam_against_enumeration_for_any_blank_and_input_kind(C, T, blank, kind):
    """test_gpu_decode.test_beam_against_enumeration with blank = 2 and all three input kinds: every labelling, against the sum
    over all C^T alignments.  Score bound: at most 5 steps of about six fp32 roundings each at magnitudes below 16 (half an ulp is
    1e-6): 3e-5 in the worst case, held to 5e-5."""
    rng = np.random.default_rng(1000 + 100 * C + 10 * T + blank)
    B = 4
    x = K.as_kind(K.random_logits(rng, B, C, T, 1.5), kind)
    got = _beam(x, 64, blank, kind=kind)
    labels = np.zeros((B, 64, T), dtype=np.int64)
    lengths = np.zeros((B, 64), dtype=np.int64)
    scores = np.full((B, 64), -np.inf)
    for b in range(B):
        exact = sorted(R.exact_labelling_log_probs(x[b], blank, kind).items(), key=lambda kv: -kv[1])
        assert len(exact) < 64
        for w, (l, v) in enumerate(exact):
            labels[b, w, :len(l)], lengths[b, w], scores[b, w] = l, len(l), v
    assert R.match_beams((labels, lengths, scores), got[:3], C, blank, np.full(B, -np.inf)) >= K.MIN_SHARE
    fin = np.isfinite(scores)
    assert np.abs(got[2][fin] - scores[fin]).max() < 5e-5
    _check_structure(got, C, blank, None)


@pytest.mark.parametrize("name", ["peak60", "long_flat"])
def test_beam_scores_far_from_zero(name):
    """peak60: every class but one near -60 in log space.  long_flat: 4096 near-uniform frames, scores about -3290 -- the float64
    sum of the per-step offsets; the relative part of the bound carries it."""
    c = K.beam_case(name)
    gl, gn, gs, gf = _check_case(c)
    if name == "long_flat":
        assert -3400.0 < gs[0, 0] < -3200.0


@pytest.mark.parametrize("name", ["integers", "fixed_point"])
def test_beam_does_not_see_an_exact_shift_of_the_logits(name):
    """logits + 1024.0, exact in fp32: both results match the reference, and each other within the same bound"""
    plain, shifted = K.beam_case(name), K.beam_case(name + "_shifted")
    a = _check_case(plain)
    b = _check_case(shifted)
    want, nxt = plain.want()
    assert R.match_beams(want, b[:3], plain.C, plain.blank, nxt) >= K.MIN_SHARE     # against the reference of the unshifted logits
    fin = np.isfinite(a[2])
    assert np.array_equal(np.isfinite(b[2]), fin)
    assert (np.abs(a[2][fin] - b[2][fin]) <= R.score_bound(want[2][fin])).all()


def _ragged_batch(seed, B, C, T):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy((rng.normal(size=(B, C, T)) * 2.0).astype(np.float32))
    lens = rng.integers(0, T + 1, size=B)
    lens[:4] = (T, 0, 1, T - 1)
    return x, torch.from_numpy(lens.astype(np.int64))


def test_an_utterance_decodes_the_same_alone_as_in_a_batch():
    D = _D()
    x, lens = _ragged_batch(7, 33, 5, 70)
    xd = x.to(DEV)
    beam = D.ctc_beam_decode(xd, 8, input_lengths=lens)
    greedy = D.ctc_greedy_decode(xd, input_lengths=lens)
    for b in range(33):
        alone = D.ctc_beam_decode(xd[b:b + 1], 8, input_lengths=lens[b:b + 1])
        for u, v in zip(alone, beam):
            assert torch.equal(u[0], v[b]), b
        alone = D.ctc_greedy_decode(xd[b:b + 1], input_lengths=lens[b:b + 1])
        for u, v in zip(alone, greedy):
            assert torch.equal(u[0], v[b]), b
    assert torch.isfinite(beam[2][:, 0]).all()
    _no_flag()


def test_strided_views_decode_as_their_contiguous_copies():
    """a channel slice of a wider tensor, every second frame of a longer one, the (B, T, C) transpose: read in place through
    the strides, bitwise equal to the contiguous copy, in both decoders"""
    D = _D()
    B, C, T = 5, 5, 70
    rng = np.random.default_rng(8)
    lens = torch.tensor([70, 33, 0, 64, 69])
    wide = torch.from_numpy((rng.normal(size=(B, 11, T)) * 2.0).astype(np.float32)).to(DEV)
    long = torch.from_numpy((rng.normal(size=(B, C, 2 * T)) * 2.0).astype(np.float32)).to(DEV)
    for view in (wide[:, 3:8, :], long[:, :, ::2]):
        assert not view.is_contiguous() and view.shape == (B, C, T)
        copy = view.contiguous()
        want_b = D.ctc_beam_decode(copy, 8, input_lengths=lens)
        want_g = D.ctc_greedy_decode(copy, input_lengths=lens)
        btc = copy.transpose(1, 2).contiguous()
        results = [(D.ctc_beam_decode(view, 8, input_lengths=lens), D.ctc_greedy_decode(view, input_lengths=lens)),
                   (D.ctc_beam_decode(btc, 8, input_lengths=lens, layout="BTC"), D.ctc_greedy_decode(btc, input_lengths=lens, layout="BTC")),
                   (D.ctc_beam_decode(view.transpose(1, 2), 8, input_lengths=lens, layout="BTC"),
                    D.ctc_greedy_decode(view.transpose(1, 2), input_lengths=lens, layout="BTC"))]
        for got_b, got_g in results:
            for u, v in zip(got_b, want_b):
                assert torch.equal(u, v)
            for u, v in zip(got_g, want_g):
                assert torch.equal(u, v)
        assert (want_b[1][:, 0] > 0).sum() == 4 and (want_g[1] > 0).sum() == 4
    _no_flag()


# -------------------------------------------------------------------------------------------------------------------- greedy

def _check_greedy(x, blank, lens):
    D = _D()
    want_l, want_f, want_n = R.greedy_decode_batch(x, blank, lens)
    xd = torch.from_numpy(x).to(DEV)
    tl = None if lens is None else torch.from_numpy(np.asarray(lens))
    for layout in ("BCT", "BTC"):
        labels, lengths, frames = D.ctc_greedy_decode(xd if layout == "BCT" else xd.transpose(1, 2).contiguous(), blank=blank,
                                                      input_lengths=tl, layout=layout)
        assert np.array_equal(lengths.cpu().numpy(), want_n)
        assert np.array_equal(labels.cpu().numpy(), want_l)
        assert np.array_equal(frames.cpu().numpy(), want_f)
    return want_l, want_f, want_n


def test_greedy_at_constructed_wave_and_chunk_boundaries():
    """blank = 3: one label over frames 62-65 (the 64-lane wave boundary), over 254-257 and 511-512 (the 256-frame chunk
    boundary), a blank at frame 255 between two runs of one label, lengths 255 / 256 / 257 through them"""
    x, lens, blank, path = K.greedy_boundaries()
    want_l, want_f, want_n = _check_greedy(x, blank, lens)
    assert want_f[0, :4].tolist() == [62, 100, 254, 511] and want_f[3, :4].tolist() == [62, 100, 250, 256]
    _no_flag()


@pytest.mark.parametrize("C,blank", [(2, 0), (2, 1), (64, 0), (64, 63), (64, 17)])
def test_greedy_at_two_and_64_classes(C, blank):
    x = K.greedy_random(100 + C + blank, 4, C, 700)
    want_l, _, want_n = _check_greedy(x, blank, np.array([700, 513, 0, 256]))
    if C == 64:
        assert want_l.max() == 63 or blank == 63
    _no_flag()


def test_greedy_with_minus_infinity():
    """-inf entries lose every comparison; a frame of nothing but -inf gives class 0, as np.argmax"""
    x = K.greedy_random(9, 3, 5, 600, with_neg_inf=True)
    for blank in (0, 2):
        _check_greedy(x, blank, None)
    labels, frames, n = R.greedy_decode_batch(x, 2)
    for b in range(3):                                               # with blank = 2, class 0 is a label: the all -inf frames emit it
        at = frames[b, :n[b]].tolist()
        assert labels[b, at.index(5)] == 0 and labels[b, at.index(300)] == 0
    _no_flag()
