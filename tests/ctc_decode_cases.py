"""The inputs of tests/test_gpu_decode_edges.py, built on the CPU from fixed seeds (numpy only), each with its reference
(tests/ctc_decode_ref.py) computed once and shared.  tests/test_ctc_decode.py checks on these very inputs, with the reference alone,
that ctc_decode_ref.match_beams would check the labelling of at least MIN_SHARE of the finite beams: the generators and seeds
below are chosen so that near-ties (reference score gaps of at most ctc_decode_ref.TIE_GAP at the pruning edge) stay rare."""
import functools

import numpy as np

from tests import ctc_decode_ref as R

MIN_SHARE = 0.90
RAGGED_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 100)      # around the 32-frame staging chunk of the beam kernel


def random_logits(rng, B, C, T, scale):
    return rng.normal(size=(B, C, T)) * scale


def peaked_path(rng, C, T, max_dwell=5):
    """a random path of runs over all C classes (the blank among them), dwells 1..max_dwell"""
    path, t = np.zeros(T, dtype=np.int64), 0
    while t < T:
        d = int(rng.integers(1, max_dwell + 1))
        path[t:t + d] = int(rng.integers(0, C))
        t += d
    return path


def peaked_logits(rng, paths, C, margin=5.0):
    """'trained-looking' output: every run of `paths` [B, T] a random 0.6-1.0 of `margin` above unit noise"""
    paths = np.asarray(paths)
    B, T = paths.shape
    x = rng.normal(size=(B, C, T))
    for b in range(B):
        t = 0
        while t < T:
            e = t
            while e < T and paths[b, e] == paths[b, t]:
                e += 1
            x[b, paths[b, t], t:e] += margin * rng.uniform(0.6, 1.0)
            t = e
    return x


def _softmax64(x):
    z = np.exp(x - x.max(axis=1, keepdims=True))
    return z / z.sum(axis=1, keepdims=True)


def as_kind(logits, kind):
    """float64 logits [B, C, T] -> the float32 input of that kind; log_probs is the log of the float32 probabilities, so that
    zeros become -inf and both forms describe the same distribution"""
    if kind == "logits":
        return logits.astype(np.float32)
    p = _softmax64(logits).astype(np.float32)
    if kind == "probs":
        return p
    with np.errstate(divide="ignore"):
        return np.log(p.astype(np.float64)).astype(np.float32)


def probs_as_kind(p, kind):
    p = np.asarray(p, dtype=np.float32)
    if kind == "probs":
        return p
    with np.errstate(divide="ignore"):
        return np.log(p.astype(np.float64)).astype(np.float32)


class BeamCase(object):
    """x [B, C, T] float32 in the form `kind` names, beam width, blank, input_lengths (or None); `truth`: the known labelling of
    utterance 0 (or None).  ref() = (labels, frames, lengths, scores, next_scores) of the reference, computed once."""

    def __init__(self, name, x, W, blank=0, kind="logits", input_lengths=None, truth=None):
        assert x.dtype == np.float32 and x.ndim == 3
        self.name, self.x, self.W, self.blank, self.kind, self.truth = name, x, W, blank, kind, truth
        self.input_lengths = None if input_lengths is None else np.asarray(input_lengths, dtype=np.int64)
        self.B, self.C, self.T = x.shape
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = R.beam_decode_batch(self.x, self.W, self.blank, self.input_lengths, self.kind, with_next=True)
        return self._ref

    def want(self):
        l, f, n, s, nxt = self.ref()
        return (l, n, s), nxt


# ---- builders: name -> BeamCase

def _limits(name, seed, peaked):
    """C = 64, W = 64, 2 utterances of 96 frames.  peaked: utterance 0 walks a permutation of all 63 non-blank classes (33 runs of
    two frames, 30 of one), utterance 1 a random path with dwells 1-5; random: scale 3"""
    rng = np.random.default_rng(seed)
    C, T = 64, 96
    if not peaked:
        return BeamCase(name, as_kind(random_logits(rng, 2, C, T, 3.0), "logits"), 64)
    order = rng.permutation(np.arange(1, C))
    dwell = rng.permutation(np.array([2] * 33 + [1] * 30))
    p0 = np.repeat(order, dwell)
    assert p0.shape == (T,)
    x = peaked_logits(rng, np.stack([p0, peaked_path(rng, C, T)]), C)
    return BeamCase(name, as_kind(x, "logits"), 64, truth=R.collapse(p0))


def _two_classes(name, seed):
    rng = np.random.default_rng(seed)
    return BeamCase(name, as_kind(random_logits(rng, 2, 2, 200, 1.5), "logits"), 64)


def _odd_width(name, seed, W, C):
    rng = np.random.default_rng(seed)
    T = 150
    if C == 7:
        x = random_logits(rng, 2, C, T, 3.0)
    else:
        x = peaked_logits(rng, np.stack([peaked_path(rng, C, T) for _ in range(2)]), C)
    return BeamCase(name, as_kind(x, "logits"), W)


def _other_blank(name, seed, blank, kind):
    """C = 5, 200 frames, W = 8.  Utterance 0 is strongly peaked (margin 12-20) on a path through every class, class 0 among the
    labels; utterance 1 is peaked as the others are, utterance 2 random at scale 3."""
    rng = np.random.default_rng(seed)
    C, T = 5, 200
    paths = np.stack([peaked_path(rng, C, T), peaked_path(rng, C, T), peaked_path(rng, C, T)])
    x = peaked_logits(rng, paths, C)
    x[0] = peaked_logits(rng, paths[:1], C, margin=20.0)[0]
    x[2] = random_logits(rng, 1, C, T, 3.0)[0]
    truth = R.collapse(paths[0], blank)
    assert 0 in truth and blank not in truth
    return BeamCase(name, as_kind(x, kind), 8, blank=blank, kind=kind, truth=truth)


def _ragged(name, seed):
    """12 utterances of 100 frames, lengths RAGGED_LENGTHS; past each length the input is garbage of magnitude 30-60 that
    favours one class per frame: a decoder that reads a frame of it ends on other prefixes and scores"""
    rng = np.random.default_rng(seed)
    B, C, T = len(RAGGED_LENGTHS), 5, 100
    x = peaked_logits(rng, np.stack([peaked_path(rng, C, T) for _ in range(B)]), C)
    x[1::2] = random_logits(rng, B // 2, C, T, 3.0)
    for b, n in enumerate(RAGGED_LENGTHS):
        x[b, :, n:] = rng.uniform(30.0, 60.0, size=(C, T - n)) * rng.choice([-1.0, 1.0], size=(C, T - n))
    return BeamCase(name, as_kind(x, "logits"), 8, input_lengths=RAGGED_LENGTHS)


def _zeros(name, seed, kind):
    """C = 5, 60 frames, W = 16, probabilities with exact zeros (kind log_probs: -inf):
      0  the blank at 0 in every frame
      1  class 3 at 0 in frames 20..39
      2  one-hot frames, but for three frames that split 0.6 / 0.4 between two classes: fewer live prefixes than W
      3  as utterance 4, with frame 30 all zero: nothing survives it
      4  no zeros"""
    rng = np.random.default_rng(seed)
    C, T = 5, 60
    p = _softmax64(random_logits(rng, 5, C, T, 2.0))
    p[0, 0] = 0.0
    p[0] /= p[0].sum(axis=0, keepdims=True)
    p[1, 3, 20:40] = 0.0
    p[1] /= p[1].sum(axis=0, keepdims=True)
    path = peaked_path(rng, C, T)
    p[2] = 0.0
    p[2, path, np.arange(T)] = 1.0
    for t in (7, 31, 32):
        c = int(path[t])
        p[2, c, t], p[2, (c + 1 + int(rng.integers(0, C - 1))) % C, t] = 0.6, 0.4
    p[3] = p[4]
    p[3, :, 30] = 0.0
    return BeamCase(name, probs_as_kind(p, kind), 16, kind=kind)


def _exact_ties(name, seed):
    """the no-pruning regime (C = 4, T = 3, W = 64: at most 40 labellings) with identical columns for classes 2 and 3: two
    prefixes that differ by swapping 2 and 3 tie bitwise, so their order is the candidate-key rule's"""
    rng = np.random.default_rng(seed)
    x = random_logits(rng, 4, 4, 3, 1.5)
    x[:, 3] = x[:, 2]
    return BeamCase(name, as_kind(x, "logits"), 64)


def _peak60(name, seed):
    """one class 60 above the others in every frame: every other class near -60 in log space"""
    rng = np.random.default_rng(seed)
    B, C, T = 2, 5, 100
    x = random_logits(rng, B, C, T, 1.0)
    paths = np.stack([peaked_path(rng, C, T) for _ in range(B)])
    x[np.arange(B)[:, None], paths, np.arange(T)[None, :]] += 60.0
    return BeamCase(name, as_kind(x, "logits"), 8)


def _long_flat(name, seed):
    """4096 near-uniform frames: scores about -3290, the sum of 4096 per-step offsets"""
    rng = np.random.default_rng(seed)
    return BeamCase(name, as_kind(random_logits(rng, 1, 5, 4096, 0.1), "logits"), 4)


SHIFT = 1024.0


def _integers(name, seed, shift):
    """integer-valued logits in [-3, 3] in the no-pruning regime (C = 4, T = 3, W = 64); with shift, SHIFT is added to every
    logit: exact in fp32, and softmax does not see it.  Integer logits tie exactly all over (the scores of two alignments differ
    by an integer, often 0), which is harmless only where nothing is pruned: match_beams compares a tie run as a set."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=(4, 4, 3)).astype(np.float64)
    return BeamCase(name, as_kind(x + (SHIFT if shift else 0.0), "logits"), 64)


def _fixed_point(name, seed, shift):
    """the same at a size that prunes (C = 5, T = 100, W = 8): logits that are multiples of 2^-8, so x + SHIFT is still exact in
    fp32 while exact ties are as rare as for random input"""
    rng = np.random.default_rng(seed)
    x = np.round(random_logits(rng, 2, 5, 100, 2.0) * 256.0) / 256.0
    return BeamCase(name, as_kind(x + (SHIFT if shift else 0.0), "logits"), 8)


BEAM_CASES = {}


def _add(name, build, *args):
    BEAM_CASES[name] = (build, args)


_add("limits_peaked", _limits, 11, True)
_add("limits_random", _limits, 12, False)
_add("two_classes", _two_classes, 21)
ODD_WIDTHS = [(W, C) for C in (7, 17) for W in (2, 3, 5, 7, 33, 63)]
for _W, _C in ODD_WIDTHS:
    _add("odd_W%d_C%d" % (_W, _C), _odd_width, 3000 + 100 * _C + _W, _W, _C)
OTHER_BLANKS = [(blank, kind) for blank in (2, 4) for kind in ("logits", "probs")]
for _blank, _kind in OTHER_BLANKS:
    _add("blank%d_%s" % (_blank, _kind), _other_blank, 40 + _blank, _blank, _kind)
_add("ragged", _ragged, 51)
for _kind in ("probs", "log_probs"):
    _add("zeros_%s" % _kind, _zeros, 61, _kind)
_add("exact_ties", _exact_ties, 71)
_add("peak60", _peak60, 81)
_add("long_flat", _long_flat, 82)
for _shift in (False, True):
    _add("integers" + "_shifted" * _shift, _integers, 83, _shift)
    _add("fixed_point" + "_shifted" * _shift, _fixed_point, 84, _shift)


@functools.lru_cache(maxsize=None)
def beam_case(name):
    build, args = BEAM_CASES[name]
    return build(name, *args)


# ---- greedy

def greedy_boundaries():
    """blank = 3, C = 5, T = 600: runs of one label across the wave boundary (frames 62-65), across the 256-frame chunk boundary
    (254-257) and (511-512), and, in utterances 3-5, a blank at frame 255 between two runs of label 1 (two emissions).  Lengths
    255, 256, 257 cut through the chunk boundary.  Returns (x [6, 5, 600] float32, input_lengths)."""
    rng = np.random.default_rng(91)
    B, C, T, blank = 6, 5, 600, 3
    path = np.full((B, T), blank, dtype=np.int64)
    path[:, 62:66] = 2
    path[:, 100:110] = 0                                             # class 0 is a label here
    path[:3, 254:258] = 4
    path[3:, 250:255] = 1
    path[3:, 256:260] = 1
    path[:, 511:513] = 1
    x = rng.normal(size=(B, C, T)) * 0.1
    x[np.arange(B)[:, None], path, np.arange(T)[None, :]] += 5.0
    return x.astype(np.float32), np.array([600, 255, 256, 257, 255, 256], dtype=np.int64), blank, path


def greedy_random(seed, B, C, T, with_neg_inf=False):
    """random logits; with_neg_inf: a fifth of the entries -inf, frames 5 and 300 all -inf (argmax 0, as np.argmax) after a
    frame of class 1"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, C, T)).astype(np.float32)
    if with_neg_inf:
        x[rng.random(size=x.shape) < 0.2] = -np.inf
        x[:, :, 5] = -np.inf
        x[:, :, 300] = -np.inf
        x[:, 1, 4] = x[:, 1, 299] = 10.0
    return x
