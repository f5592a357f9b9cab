"""Inputs of the signal_align tests, built once (seeded numpy), with their references from tests/signal_align_ref.py cached per
case.  A case is a batch of reads drawn from an integer pore model: random bases, a dwell per k-mer, and every sample its k-mer's
level plus Gaussian noise of its stdv.  The integer model [4^k, 3] is written down here directly (level = round(mean 2^F), weight
= round(2^(S + 8) / (2 (stdv 2^F)^2)) at a fixed S = 40, offset = round(2^8 ln(stdv 2^F))), without the package: the GPU tests pass
it as a hand-filled SignalModel."""
import collections
import functools

import numpy as np

from tests import signal_align_ref as R

Case = collections.namedtuple("Case", "signal signal_lengths labels label_lengths model kw true_starts")
F, S, COST_BITS = 12, 40, 8
SAMPLE_CHUNK = 1024                     # csrc/wn_sigalign.hip: kSaSamples


@functools.lru_cache(maxsize=None)
def table(k, seed=3):
    rng = np.random.default_rng(seed + k)
    n = 4 ** k
    means, stdvs = 70.0 + 40.0 * rng.random(n), 1.0 + 2.0 * rng.random(n)
    model = np.empty((n, 3), dtype=np.int64)
    model[:, 0] = np.rint(means * 2.0 ** F)
    model[:, 1] = np.rint(2.0 ** (S + COST_BITS) / (2.0 * (stdvs * 2.0 ** F) ** 2))
    model[:, 2] = np.rint(2.0 ** COST_BITS * np.log(stdvs * 2.0 ** F))
    return means, stdvs, model


def build(seed, dwell_rows, k=5, first=0, band=64, model=None, levels=None, labels=None, pad=3, **more):
    """dwell_rows: per read the samples of each state.  levels: (means, stdvs) to draw from instead of table(k)"""
    rng = np.random.default_rng(seed)
    means, stdvs, tab = table(k)
    if levels is not None:
        means, stdvs = levels
    B = len(dwell_rows)
    n_states = [len(r) for r in dwell_rows]
    ll = np.array([n + (k - 1) + 2 * first for n in n_states], dtype=np.int32)
    if labels is None:
        labels = rng.integers(1, 5, size=(B, int(ll.max()))).astype(np.int32)
    T = np.array([int(np.sum(r)) for r in dwell_rows], dtype=np.int32)
    L = int(T.max()) + pad
    signal = (90.0 + 12.0 * rng.standard_normal((B, L))).astype(np.float32)
    true_starts = np.zeros((B, max(n_states) + 1), dtype=np.int32)
    for b, row in enumerate(dwell_rows):
        codes = R.read_states(labels[b], int(ll[b]), k, first)
        edges = np.concatenate([[0], np.cumsum(row)]).astype(np.int32)
        true_starts[b, :len(edges)] = edges
        true_starts[b, len(edges):] = edges[-1]
        which = np.repeat(np.asarray(codes, dtype=np.int64), row)
        signal[b, :T[b]] = (means[which] + stdvs[which] * rng.standard_normal(T[b])).astype(np.float32)
    kw = dict(dict(k=k, first=first, band=band, frac_bits=F, weight_shift=S, max_cost=None), **more)
    return Case(signal, T, labels, ll, tab if model is None else model, kw, true_starts)


def _dwell(rng, n, lo, hi):
    return rng.integers(lo, hi, size=n).tolist()


# ---- the case worked by hand (tests/test_signal_align_ref.py): k = 1, F = 0, cost = d^2
HAND_MODEL = np.array([[10, 1 << 16, 0], [20, 1 << 16, 0], [30, 1 << 16, 0], [40, 1 << 16, 0]], dtype=np.int64)
HAND_KW = dict(k=1, first=0, band=64, frac_bits=0, weight_shift=16, max_cost=None)


def hand_case():
    signal = np.array([[10, 14, 16, 20, 26, 30, 99]], dtype=np.float32)
    return Case(signal, np.array([6], np.int32), np.array([[1, 2, 3]], np.int32), np.array([3], np.int32), HAND_MODEL, HAND_KW,
                np.array([[0, 2, 4, 6]], np.int32))


def homopolymer_case():
    """constant signal over one repeated base: every path ties"""
    signal = np.full((2, 33), 20.0, dtype=np.float32)
    return Case(signal, np.array([30, 10], np.int32), np.full((2, 10), 2, np.int32), np.array([10, 10], np.int32), HAND_MODEL, HAND_KW,
                None)


def dyadic_case():
    """two levels 64 apart, samples on a level or half way between: costs 0, 1024 and 4096 only, so many paths tie"""
    rng = np.random.default_rng(31)
    model = np.array([[64, 1 << 16, 0], [128, 1 << 16, 0], [64, 1 << 16, 0], [128, 1 << 16, 0]], dtype=np.int64)
    labels = rng.integers(1, 3, size=(3, 50)).astype(np.int32)
    signal = rng.choice(np.array([64.0, 96.0, 128.0], dtype=np.float32), size=(3, 203))
    return Case(signal, np.array([200, 173, 50], np.int32), labels, np.array([50, 50, 50], np.int32), model, HAND_KW, None)


def _cases():
    rng = np.random.default_rng(11)
    c = {"hand": hand_case(), "homopolymer": homopolymer_case(), "dyadic": dyadic_case()}
    # one state; as many samples as states; one sample too few; no samples; labels shorter than k + 2 first (N = 0 and N = -1)
    small = build(1, [[5], [1] * 7, [1] * 6, [2, 3], [1], [1]], k=3, first=1)
    small.signal_lengths[2] = 5
    small.signal_lengths[3] = 0
    small.label_lengths[4], small.label_lengths[5] = 4, 3
    c["small"] = small
    c["band_never_moves"] = build(2, [_dwell(rng, 40, 3, 13)], band=64)
    c["moving_band"] = build(3, [_dwell(rng, 300, 4, 9)], band=64, first=2)
    for W in (64, 512, 576, 2048):
        c["threads_w%d" % W] = build(4, [_dwell(np.random.default_rng(41), 2200, 1, 4)], band=W)
    edge = []
    for T in (SAMPLE_CHUNK - 1, SAMPLE_CHUNK, SAMPLE_CHUNK + 1, 2 * SAMPLE_CHUNK - 1, 2 * SAMPLE_CHUNK, 2 * SAMPLE_CHUNK + 1):
        row = _dwell(rng, 200, 3, 6)
        row[-1] += T - sum(row)
        edge.append(row)
    c["sample_chunk_edges"] = build(5, edge, band=64, pad=0)
    c["long_read"] = build(6, [_dwell(rng, 9000, 6, 10)], band=64)
    half = [1] * 200 + _dwell(rng, 200, 7, 12)
    c["pressed_w64"] = build(7, [half], band=64)
    c["pressed_w2048"] = build(7, [half], band=2048)
    outlier = build(8, [_dwell(rng, 5, 4, 9), _dwell(rng, 5, 4, 9)], k=2, max_cost=5000)
    outlier.signal[0, 11] = 1000.0
    outlier.signal[1, 0] = -2000.0
    c["cost_clamp"] = outlier
    for k, first in ((1, 0), (1, 2), (5, 0), (5, 2), (6, 0), (6, 2)):
        c["form_k%d_first%d" % (k, first)] = build(20 + 3 * k + first, [_dwell(rng, 100, 2, 8), _dwell(rng, 37, 1, 5), _dwell(rng, 64, 3, 4)],
                                                   k=k, first=first)
    return c


CASES = _cases()


def call_ref(case, band="kw", signal=None, scale_shift=None):
    kw = dict(case.kw)
    if band != "kw":
        kw["band"] = band
    return R.signal_align_ref(case.signal if signal is None else signal, case.signal_lengths, case.labels, case.label_lengths, case.model,
                              scale_shift=scale_shift, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    return call_ref(CASES[name])


def int16_of(case):
    """(raw int16 [B, L], scale_shift float32 [B, 2]) of a case of any of the signal tools: the samples in eighths, under a scale
    near 1/8 and a shift, both seeded"""
    rng = np.random.default_rng(99)
    raw = np.rint(case.signal.astype(np.float64) * 8.0).astype(np.int16)
    B = raw.shape[0]
    ss = np.stack([0.125 * (1.0 + 0.01 * rng.standard_normal(B)), 3.0 * rng.standard_normal(B)], axis=1).astype(np.float32)
    return raw, ss


@functools.lru_cache(maxsize=None)
def int16_form(name):
    return int16_of(CASES[name])


@functools.lru_cache(maxsize=None)
def int16_reference(name):
    raw, ss = int16_form(name)
    return call_ref(CASES[name], signal=raw, scale_shift=ss)


# ---- every fault once, between good reads: 30 states of 3..7 samples, k = 5, first = 2
BAD_READS = ("good", "signal_length_above", "signal_length_negative", "label_length_above", "label_length_negative", "label_0",
             "label_5", "good_label_0_before_the_window", "nan", "inf", "range", "weight_0", "good_nan_past_the_read", "good_at_the_limit")
BAD_GOOD = {"good", "good_label_0_before_the_window", "good_nan_past_the_read", "good_at_the_limit"}


@functools.lru_cache(maxsize=None)
def bad_batch():
    rng = np.random.default_rng(21)
    case = build(22, [_dwell(rng, 30, 3, 8) for _ in BAD_READS], k=5, first=2, pad=4)
    signal, labels, sl, ll = case.signal.copy(), case.labels.copy(), case.signal_lengths.copy(), case.label_lengths.copy()
    model = case.model.copy()
    r = BAD_READS.index
    sl[r("signal_length_above")] = signal.shape[1] + 1
    sl[r("signal_length_negative")] = -1
    ll[r("label_length_above")] = labels.shape[1] + 1
    ll[r("label_length_negative")] = -1
    labels[r("label_0"), 2] = 0                                       # the first label of the window
    labels[r("label_5"), ll[r("label_5")] - 3] = 5                    # the last one
    labels[r("good_label_0_before_the_window"), 1] = 0
    labels[r("good_label_0_before_the_window"), ll[r("good")] - 2] = 7
    signal[r("nan"), 17] = np.nan
    signal[r("inf"), 0] = -np.inf
    signal[r("range"), sl[r("range")] - 1] = 2048.0                   # 2048 * 2^12 = 2^23: the first value out of range
    signal[r("good_at_the_limit"), 40] = 2047.99
    signal[r("good_nan_past_the_read"), sl[r("good_nan_past_the_read")]:] = np.nan
    own = set(R.read_states(labels[r("weight_0")], int(ll[r("weight_0")]), 5, 2))
    for b, name in enumerate(BAD_READS):
        if name in BAD_GOOD:
            own -= set(R.read_states(labels[b], int(case.label_lengths[b]), 5, 2))
    model[min(own), 1] = 0                                            # a k-mer only the faulty read uses
    return Case(signal, sl, labels, ll, model, case.kw, case.true_starts)


@functools.lru_cache(maxsize=None)
def bad_reference():
    return call_ref(bad_batch())


@functools.lru_cache(maxsize=None)
def garbage_batch(seed):
    """lengths anywhere in the int32 range, labels -3..8, NaN and huge samples, a model with rows out of range"""
    rng = np.random.default_rng(seed)
    B, L, n = 24, 90, 40
    signal = (90.0 + 12.0 * rng.standard_normal((B, L))).astype(np.float32)
    signal[rng.random((B, L)) < 0.01] = np.nan
    signal[rng.random((B, L)) < 0.01] = 3e9
    sl = rng.integers(-2 ** 31, 2 ** 31, size=B).astype(np.int32)
    ll = rng.integers(-2 ** 31, 2 ** 31, size=B).astype(np.int32)
    sl[::3] = rng.integers(0, L + 1, size=len(sl[::3]))
    ll[::2] = rng.integers(0, n + 1, size=len(ll[::2]))
    labels = rng.integers(-3, 9, size=(B, n)).astype(np.int32)
    labels[::4] = rng.integers(1, 5, size=labels[::4].shape)
    model = table(3)[2].copy()
    model[rng.integers(0, 64, 6), 1] = rng.integers(-5, 1, 6)
    model[rng.integers(0, 64, 3), 0] = 1 << 23
    model[rng.integers(0, 64, 3), 2] = -(1 << 30)
    return Case(signal, sl, labels, ll, model, dict(k=3, first=1, band=64, frac_bits=F, weight_shift=S, max_cost=70000), None)
