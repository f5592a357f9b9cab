"""Inputs of the signal_map tests, built once (seeded numpy), with their references from tests/signal_map_ref.py cached per case.
A case is a reference (bases 0..4), an integer pore model and a batch of reads; a read's samples follow a random stretch of the
reference (a dwell per state, the state's level plus Gaussian noise), so that there is a locus to find, or are what the case says.
The integer models are those of tests/signal_align_cases.py (table(k) at S = 40, F = 12, and the hand model with cost d^2)."""
import collections
import functools
import random

import numpy as np

from tests import signal_align_cases as A
from tests import signal_map_ref as R

Case = collections.namedtuple("Case", "signal signal_lengths ref model kw truth")
F, S, COST_BITS = A.F, A.S, A.COST_BITS
TILE = 1024                             # csrc/wn_sigmap.hip: kSmTile, a power of two
SWEEP_M = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4100)
SWEEP_T = (1, 2, 3, 65, 700)
STRIPS = (64, 128, 576, None)


def build(seed, ref, lengths, k=3, pad=3, noise=1.0, **more):
    """reads of `lengths` samples, each along a random stretch of `ref` that holds no wall (where there is one)"""
    rng = np.random.default_rng(seed)
    means, stdvs, model = A.table(k)
    codes, _ = R.prepare(ref, model, k)
    M, B = len(codes), len(lengths)
    L = max(max(lengths), 1) + pad
    signal = (90.0 + 12.0 * rng.standard_normal((B, L))).astype(np.float32)
    truth = np.full(B, -1, dtype=np.int64)
    for b, T in enumerate(lengths):
        dwell = rng.integers(1, 4, size=T + 1)
        states = np.repeat(np.arange(T + 1), dwell)[:T]              # at most T states
        for _ in range(20):
            s0 = int(rng.integers(0, max(M - int(states[-1] if T else 0), 1)))
            path = s0 + states
            if T and path[-1] < M and (codes[path] >= 0).all():
                signal[b, :T] = (means[codes[path]] + noise * stdvs[codes[path]] * rng.standard_normal(T)).astype(np.float32)
                truth[b] = s0
                break
    kw = dict(dict(k=k, frac_bits=F, weight_shift=S, max_cost=None), **more)
    return Case(signal, np.asarray(lengths, dtype=np.int32), np.asarray(ref, dtype=np.int32), model, kw, truth)


def random_ref(seed, M, k, breaks=0.0):
    rng = np.random.default_rng(seed)
    ref = rng.integers(1, 5, size=M + k - 1)
    if breaks:
        ref[rng.random(len(ref)) < breaks] = 0
    return ref.astype(np.int32)


# ---- the case worked by hand (tests/test_signal_map_ref.py): k = 1, F = 0, cost = d^2, levels 10 20 30 40
HAND_KW = dict(k=1, frac_bits=0, weight_shift=16, max_cost=None)


def hand_case():
    return Case(np.array([[20, 21, 30, 29, 99]], dtype=np.float32), np.array([4], np.int32), np.array([1, 2, 3, 4, 1], np.int32),
                A.HAND_MODEL, HAND_KW, None)


def homopolymer_case():
    """one repeated base and a constant signal: every cell of the last row is equal, the smallest end wins and its path never
    stepped"""
    return Case(np.full((2, 133), 20.0, dtype=np.float32), np.array([5, 130], np.int32), np.full(3000, 2, np.int32), A.HAND_MODEL,
                HAND_KW, None)


def two_copies_case():
    """a 150-base locus at 200 and again at 2500 (another strip at every strip of STRIPS, another tile), the reads drawn from it:
    both copies cost the same to the last bit, the left one wins"""
    rng = np.random.default_rng(51)
    ref = random_ref(52, 4100, 3)
    ref[2500:2650] = ref[200:350]
    case = build(53, ref[200:350], [60, 200], k=3)                   # reads along the locus alone
    signal = np.concatenate([case.signal, (90.0 + 12.0 * rng.standard_normal((1, case.signal.shape[1]))).astype(np.float32)])
    return Case(signal, np.array([60, 200, 100], np.int32), ref, case.model, case.kw, case.truth + 200)


def seam_walls_case():
    """breaks on strip seams (64, 128, 576 and their multiples) and on the tile seam: the states whose windows hold them are walls"""
    ref = random_ref(54, 4100, 3)
    for pos in (63, 64, 128, 575, 576, 577, 1022, 1023, 1024, 1025, 1152, 2048, 2049, 3071, 3072, 4099):
        ref[pos] = 0
    return build(55, ref, [1, 2, 3, 64, 65, 130, 300, 700], k=3)


def _cases():
    c = {"hand": hand_case(), "homopolymer": homopolymer_case(), "two_copies": two_copies_case(), "seam_walls": seam_walls_case()}
    for M in SWEEP_M:
        c["sweep_%d" % M] = build(100 + M, random_ref(200 + M, M, 3, breaks=0.004 if M > 100 else 0.0), list(SWEEP_T), k=3)
    c["strips"] = build(60, random_ref(61, 4100, 3, breaks=0.002), [1, 2, 63, 64, 65, 300, 699, 700], k=3)
    c["all_walls"] = build(62, np.zeros(600, np.int32), [1, 50], k=3)
    sparse = np.zeros(300, np.int32)                                 # open states 100..119 alone: fewer than the read has samples
    sparse[100:122] = random_ref(63, 20, 3)
    c["few_open_states"] = build(64, sparse, [10, 30], k=3)
    c["t_above_m"] = build(65, random_ref(66, 40, 3), [100, 41, 40, 39], k=3)
    c["cost_clamp"] = build(67, random_ref(68, 300, 2), [50, 50], k=2, max_cost=5000)
    c["cost_clamp"].signal[0, 11] = 1000.0
    c["cost_clamp"].signal[1, 0] = -2000.0
    for k in (1, 5, 6):
        c["form_k%d" % k] = build(70 + k, random_ref(80 + k, 1500, k, breaks=0.002), [400, 37, 129], k=k)
    return c


CASES = _cases()


def call_ref(case, signal=None, scale_shift=None):
    return R.signal_map_ref(case.signal if signal is None else signal, case.signal_lengths, case.ref, case.model,
                            scale_shift=scale_shift, **case.kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    return call_ref(CASES[name])


@functools.lru_cache(maxsize=None)
def int16_form(name):
    return A.int16_of(CASES[name])


@functools.lru_cache(maxsize=None)
def int16_reference(name):
    raw, ss = int16_form(name)
    return call_ref(CASES[name], signal=raw, scale_shift=ss)


# ---- every fault once, between good reads
BAD_READS = ("good", "length_above", "length_negative", "good_empty", "nan", "inf", "range", "good_nan_past_the_read",
             "good_at_the_limit", "good_last")
BAD_GOOD = {"good", "good_empty", "good_nan_past_the_read", "good_at_the_limit", "good_last"}


@functools.lru_cache(maxsize=None)
def bad_batch():
    case = build(90, random_ref(91, 700, 3, breaks=0.003), [120] * len(BAD_READS), k=3, pad=4)
    signal, sl = case.signal.copy(), case.signal_lengths.copy()
    r = BAD_READS.index
    sl[r("length_above")] = signal.shape[1] + 1
    sl[r("length_negative")] = -1
    sl[r("good_empty")] = 0
    signal[r("good_empty"), 0] = np.nan                               # never read
    signal[r("nan"), 17] = np.nan
    signal[r("inf"), 0] = -np.inf
    signal[r("range"), sl[r("range")] - 1] = 2048.0                   # 2048 * 2^12 = 2^23: the first value out of range
    signal[r("good_at_the_limit"), 40] = 2047.99
    signal[r("good_nan_past_the_read"), sl[r("good_nan_past_the_read")]:] = np.nan
    return Case(signal, sl, case.ref, case.model, case.kw, case.truth)


@functools.lru_cache(maxsize=None)
def bad_reference():
    return call_ref(bad_batch())


@functools.lru_cache(maxsize=None)
def faulty_reference_case():
    """a reference with a label 7 and a k-mer whose model row has weight 0: both counted, both mapped as walls"""
    base = build(92, random_ref(93, 500, 3), [80, 200], k=3)
    ref, model = base.ref.copy(), base.model.copy()
    ref[250] = 7
    codes, _ = R.prepare(ref, model, 3)
    model[int(codes[40]), 1] = 0
    return Case(base.signal, base.signal_lengths, ref, model, base.kw, None)


# ---- the 24-read fixture: regenerated from its seeds, no stored file
FIXTURE_SAMPLES = 400


@functools.lru_cache(maxsize=None)
def fixture():
    """A 3000-base reference and 24 stretches of 120 bases, each with a strand, from Python's random.seed(7); both strands joined
    by a wall; 24 reads of 120 bases cut from either strand, made by ragged_reads on the CPU under the stand-in table (dwell
    uniform in [4, 8), the generator's window, torch.Generator().manual_seed(5)); their first 400 samples.  Returns a dict:
    bases (the forward strand), joined, read_bases [24, 120], start_state [24] (in the joined sequence), strand [24], reads (the
    RaggedReads), signal [24, 400] float32, signal_lengths [24] and the stand-in model (a SignalModel)."""
    import torch

    import wavenet_speech_amd as W
    from wavenet_speech_amd import synthetic
    random.seed(7)
    bases = ["ACGT".index(random.choice("ACGT")) + 1 for _ in range(3000)]
    picks = []
    for _ in range(24):                                              # per read: its strand, then where its stretch begins
        strand = random.randrange(2)
        picks.append((random.randrange(0, 3000 - 120 + 1), strand))
    joined = R.join_strands(bases)
    start_state = np.array([p if s == 0 else 3001 + p for p, s in picks], dtype=np.int64)
    read_bases = np.array([joined[s:s + 120] for s in start_state], dtype=np.int32)
    table = synthetic.standin_kmer_table()
    reads = synthetic.ragged_reads(24, dwell=("uniform", 6, 2), window="generator", table=table, bases=torch.from_numpy(read_bases),
                                   generator=torch.Generator().manual_seed(5), device="cpu")
    signal = reads.signal[:, 0, :FIXTURE_SAMPLES].contiguous().numpy()
    lengths = reads.signal_lengths.clamp(max=FIXTURE_SAMPLES).numpy().astype(np.int32)
    return {"bases": np.array(bases, dtype=np.int32), "joined": np.array(joined, dtype=np.int32), "read_bases": read_bases,
            "start_state": start_state, "strand": np.array([s for _, s in picks]), "reads": reads, "signal": signal,
            "signal_lengths": lengths, "model": W.signal_model(*table)}


@functools.lru_cache(maxsize=None)
def fixture_reference():
    fx = fixture()
    m = fx["model"]
    return R.signal_map_ref(fx["signal"], fx["signal_lengths"], fx["joined"], m.table.numpy(), m.k, m.frac_bits, m.weight_shift)
