"""Inputs of the limit tests of the two dynamic-programming aligners (csrc/wn_align.hip, CTC forced alignment, and
csrc/wn_pairalign.hip, affine-gap pairwise alignment) and of the quality profile on their longest outputs, built once from seeds
(numpy only), with their references cached.  Nothing here is random at test time and nothing is taken from a kernel: every expected
number comes from tests/ctc_align_ref.py or tests/pairwise_align_ref.py, used as they are, or from a closed form below that
tests/test_align_limits_ref.py holds equal to those references at small sizes.  The sections follow the limits the kernels' header
comments state:

    forced aligner     1  the steepest path: +2 states on every frame, so a 64-frame trace chunk walks its whole 9-word window
                       2  several waves on a quarter grid, where ties are real and `left` crosses waves through LDS
                       3  the 64-frame chunk edges in time, as the tensor's T and as input_lengths
                       4  2 and 64 classes, the blank first, last and in the middle
                       5  log-probabilities of -inf: a band, an utterance without any alignment, and holes beside the path
    pairwise aligner   1  a row against itself: 64 diagonal lookups walk the whole 72-step x 9-thread window
                       2  the cost limits
                       3  the reference ring's reloads in one wave and in several, all 1024 threads, 9 waves
                       4  the longest stream, by closed form
    quality profile       the op strings of the longest alignments, and synthetic ones at both length limits"""
import collections
import functools

import numpy as np

from tests import ctc_align_ref as A
from tests import pairwise_align_ref as R
from tests import quality_profile_cases as PC
from tests import quality_profile_ref as PR

# ======================================================================================================= the forced aligner
# x [B, C, T] float32 log-probabilities on the quarter grid, labels: B lists, input_lengths: B ints or None (= T)
Forced = collections.namedtuple("Forced", "x labels input_lengths blank")
NEG_INF = np.float32(-np.inf)


def grid(rng, shape):
    """integers in [-24, 0] divided by 4: every float64 sum, and the float32 score, is exact (below 2^24 quarters: 699050 frames)"""
    return (rng.integers(-24, 1, size=shape) / 4.0).astype(np.float32)


def steep_labels(L):
    """no two neighbours equal: with T == L the only alignment is the states 1, 3, 5, ..."""
    return [1 + i % 4 for i in range(L)]


def repeat_labels(L):
    """steep_labels with every third label equal to the one before it: a forced blank between them"""
    labels = steep_labels(L)
    for i in range(2, L, 3):
        labels[i] = labels[i - 1]
    return labels


def forced_states(labels):
    """the only alignment of `labels` to len(labels) + (number of repeats) frames: one frame per label, one per forced blank"""
    out = []
    for j, v in enumerate(labels):
        if j and labels[j - 1] == v:
            out.append(2 * j)
        out.append(2 * j + 1)
    return np.array(out, dtype=np.int32)


STEEP_ONE_WAVE = tuple(range(64, 72))                   # T == L: the last state 2 L - 1 has all eight phases of s_end & 15
STEEP_WAVES = (255, 256, 257, 1023, 1024, 2047)
NEAR_STEEP = (71, 257, 1024)                            # T = L + 1 and L + 3 over random values: near-steepest, with a choice
LEAD_ONE_WAVE = (200, tuple(range(1, 8)))               # L, the numbers d of leading blank frames
LEAD_WAVES = (1023, (1, 4))
TIE_SHAPES = {256: 600, 300: 700, 1023: 2100, 2047: 4200}
TIE_SEEDS = {256: 7, 300: 1, 1023: 4, 2047: 0}          # the first seeds whose reference meets tests/test_align_limits_ref.py
TIME_EDGES = (1, 63, 64, 65, 127, 128, 129, 4096)
TIME_TENSOR = 4100                                      # the longer tensor the same lengths are cut out of


def _steep(seed, sizes):
    """every L plain (T = L) and with repeats (T = L + repeats) in one batch"""
    rng = np.random.default_rng(seed)
    labels = [steep_labels(L) for L in sizes] + [repeat_labels(L) for L in sizes]
    lengths = [len(forced_states(l)) for l in labels]
    return Forced(grid(rng, (len(labels), 5, max(lengths))), labels, lengths, 0)


def _near(seed, L):
    rng = np.random.default_rng(seed)
    return Forced(grid(rng, (2, 5, L + 3)), [steep_labels(L)] * 2, [L + 1, L + 3], 0)


def _lead(seed, L, leads):
    """d frames where only the blank is likely, then frame d + j likely for label j alone: the path waits in state 0 and then
    takes +2 on every frame, so a chunk's last state has the phase (15 - 2 d) & 15 and the chunk still walks 126 states down"""
    rng = np.random.default_rng(seed)
    labels = steep_labels(L)
    x = (rng.integers(-24, 0, size=(len(leads), 5, L + max(leads))) / 4.0).astype(np.float32)      # nothing at 0 ...
    for b, d in enumerate(leads):
        x[b, 0, :d] = 0.0                                                                          # ... but the planted path
        x[b, labels, d + np.arange(L)] = 0.0
    return Forced(x, [labels] * len(leads), [L + d for d in leads], 0)


def _ties(L, seed=None):
    """two utterances: the limit one, and a ragged one of L // 3 labels over fewer frames"""
    T = TIE_SHAPES[L]
    rng = np.random.default_rng(1000 * L + (TIE_SEEDS[L] if seed is None else seed))
    x = grid(rng, (2, 5, T))
    return Forced(x, [rng.integers(1, 5, size=L).tolist(), rng.integers(1, 5, size=L // 3).tolist()], [T, T - T // 5], 0)


def _time_labels(rng, T, C=5):
    return [rng.integers(1, C, size=n).tolist() for n in (0, 1, min(T // 2, 300))]


def _time(T):
    rng = np.random.default_rng(300 + T)
    return Forced(grid(rng, (3, 5, T)), _time_labels(rng, T), None, 0)


def _time_inside():
    rng = np.random.default_rng(299)
    labels, lengths = [], []
    for T in TIME_EDGES:
        labels += _time_labels(rng, T)
        lengths += [T] * 3
    return Forced(grid(rng, (len(labels), 5, TIME_TENSOR)), labels, lengths, 0)


def _two_classes(blank):
    """every label is the one class that is not the blank, so every gap between two labels is a forced blank; 350 labels in 699
    frames leave no choice at all, 300 in 700 do"""
    rng = np.random.default_rng(400 + blank)
    return Forced(grid(rng, (2, 2, 700)), [[1 - blank] * 350, [1 - blank] * 300], [699, 700], blank)


def _most_classes(blank):
    rng = np.random.default_rng(410 + blank)
    others = np.array([c for c in range(64) if c != blank])
    return Forced(grid(rng, (1, 64, 700)), [others[rng.integers(0, 63, size=300)].tolist()], None, blank)


NEG_INF_BAND = 20


def _neg_inf():
    """0: label classes are -inf wherever none of the labels within 20 of the diagonal has that class; 1: a needed class is -inf on
    every frame; 2: -inf on 30 % of the (class, frame) entries that the best path of the finite values does not use"""
    rng = np.random.default_rng(500)
    C, T = 16, 700
    x = grid(rng, (3, C, T))
    labels = [rng.integers(1, C, size=300).tolist(), rng.integers(1, C, size=40).tolist(), rng.integers(1, C, size=150).tolist()]
    for t in range(T):
        j = t * 300 // T
        near = set(labels[0][max(j - NEG_INF_BAND, 0):j + NEG_INF_BAND + 1])
        x[0, [c for c in range(1, C) if c not in near], t] = NEG_INF
    x[1, labels[1][17], :] = NEG_INF
    states, _, _ = A.viterbi_align(x[2].astype(np.float64), labels[2])
    used = A.frame_labels_of(states, labels[2])
    holes = rng.random((C, T)) < 0.3
    holes[used, np.arange(T)] = False
    x[2][holes] = NEG_INF
    return Forced(x, labels, None, 0)


FORCED = collections.OrderedDict()
FORCED["steep_one_wave"] = lambda: _steep(100, STEEP_ONE_WAVE)
for _L in STEEP_WAVES:
    FORCED["steep_L%d" % _L] = functools.partial(_steep, 100 + _L, (_L,))
for _L in NEAR_STEEP:
    FORCED["near_L%d" % _L] = functools.partial(_near, 200 + _L, _L)
FORCED["lead_one_wave"] = lambda: _lead(210, *LEAD_ONE_WAVE)
FORCED["lead_waves"] = lambda: _lead(211, *LEAD_WAVES)
for _L in sorted(TIE_SHAPES):
    FORCED["ties_L%d" % _L] = functools.partial(_ties, _L)
for _T in TIME_EDGES:
    FORCED["time_T%d" % _T] = functools.partial(_time, _T)
FORCED["time_inside"] = _time_inside
FORCED["two_classes_blank0"] = lambda: _two_classes(0)
FORCED["two_classes_blank1"] = lambda: _two_classes(1)
for _b in (0, 63, 31):
    FORCED["classes64_blank%d" % _b] = functools.partial(_most_classes, _b)
FORCED["neg_inf"] = _neg_inf


@functools.lru_cache(maxsize=None)
def forced(name):
    return FORCED[name]()


def forced_lp(case, b):
    """the float64 log-probabilities [C, Tb] of utterance b"""
    Tb = case.x.shape[2] if case.input_lengths is None else case.input_lengths[b]
    return case.x[b, :, :Tb].astype(np.float64)


@functools.lru_cache(maxsize=None)
def forced_reference(name):
    """per utterance (states, score, spans) of ctc_align_ref.viterbi_align; shared, so do not write into it"""
    case = forced(name)
    return [A.viterbi_align(forced_lp(case, b), labels, blank=case.blank) for b, labels in enumerate(case.labels)]


# ===================================================================================================== the pairwise aligner
# costs in the kernel's integer half-units: (match, mismatch, gap_open, gap_extend)
COSTS = collections.OrderedDict([
    ("emboss", R.EMBOSS),
    ("largest", (1024, -1024, 1024, 1024)),
    ("largest_free_extend", (1024, -1024, 1024, 0)),
    ("all_zero", (0, 0, 0, 0)),
    ("inverted", (-1024, 1024, 1024, 0)),
    ("all_positive", (5, 5, 3, 1)),
])
COST_LIMIT_SETS = ("largest", "largest_free_extend", "all_zero", "inverted", "all_positive")
Pairs = collections.namedtuple("Pairs", "refs queries costs")

SELF_ONE_WAVE = (1, 8, 63, 64, 65, 71, 72, 73, 128, 512)
SELF_WAVES = (513,) + tuple(range(520, 528))            # 520..527: all eight column phases of the end cell
SELF_LONG = (1100,)
SELF_GROUPS = {"one_wave": SELF_ONE_WAVE, "waves": SELF_WAVES, "long": SELF_LONG}
SELF_CLOSED = 8192
SHIFTS = (1, 7, 8, 9)
PLANTED = (64, 65, 128, 129)                            # one mismatch this far from the end
RING_N = (1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4100)
RING_M = (8, 520, 1100)
LONGEST = (65535, 8192)


def mutate(rng, ref, rate, alphabet):
    """a query made from the reference by substitutions, insertions and deletions, `rate` of the positions each way (the
    generator of tests/test_gpu_pairalign.py)"""
    out = []
    for v in ref:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(int(rng.integers(1, alphabet + 1)))
        if u > 1 - rate / 3:
            v = int(rng.integers(1, alphabet + 1))
        out.append(int(v))
    return out


def letters(rng, n, alphabet=4):
    return rng.integers(1, alphabet + 1, size=n).tolist()


def _self(seed, sizes, costs):
    rng = np.random.default_rng(seed)
    rows = [letters(rng, n) for n in sizes]
    return Pairs(rows, [list(r) for r in rows], COSTS[costs])


def _variants(seed, n, costs):
    """a row against itself but for one mismatch 64 / 65 / 128 / 129 from the end, and against itself without its first s labels,
    either way round: a long diagonal and a head gap"""
    rng = np.random.default_rng(seed)
    row = letters(rng, n)
    refs, queries = [], []
    for d in PLANTED:
        q = list(row)
        q[n - d] = q[n - d] % 4 + 1
        refs.append(row); queries.append(q)
    for s in SHIFTS:
        refs += [row, row[s:]]
        queries += [row[s:], row]
    return Pairs(refs, queries, COSTS[costs])


def _cost_pairs(seed, n, costs):
    """2-letter and 4-letter rows, each against a mutated copy and against an unrelated row of about the same length"""
    rng = np.random.default_rng(seed)
    refs, queries = [], []
    for alphabet in (2, 4):
        ref = letters(rng, n, alphabet)
        refs += [ref, ref]
        queries += [mutate(rng, ref, 0.2, alphabet), letters(rng, n - n // 11, alphabet)]
    return Pairs(refs, queries, COSTS[costs])


def stretch_query(rng, ref, M):
    """exactly M labels: a mutated stretch of the reference, filled up with random labels where the reference is too short"""
    start = int(rng.integers(0, max(len(ref) - M, 0) + 1))
    q = mutate(rng, ref[start:start + M + M // 8 + 8], 0.15, 4)[:M]
    return q + letters(rng, M - len(q))


def _ring(N):
    rng = np.random.default_rng(7000 + N)
    ref = letters(rng, N)
    return Pairs([ref] * len(RING_M), [stretch_query(rng, ref, M) for M in RING_M], R.EMBOSS)


def _wide(seed, N, M):
    """M > N: the reference is a mutated stretch of the long query"""
    rng = np.random.default_rng(seed)
    q = letters(rng, M)
    span = N + N // 8 + 8
    start = (M - span) // 2
    ref = mutate(rng, q[start:start + span], 0.15, 4)[:N]
    assert len(ref) == N
    return Pairs([ref], [q], R.EMBOSS)


PAIRS = collections.OrderedDict()
for _g, _sizes in sorted(SELF_GROUPS.items()):
    for _c in ("emboss", "largest"):
        PAIRS["self_%s/%s" % (_g, _c)] = functools.partial(_self, 600 + len(_sizes), _sizes, _c)
PAIRS["variants_200/emboss"] = functools.partial(_variants, 610, 200, "emboss")
PAIRS["variants_200/largest"] = functools.partial(_variants, 610, 200, "largest")
PAIRS["variants_600/emboss"] = functools.partial(_variants, 611, 600, "emboss")
for _c in COST_LIMIT_SETS:
    PAIRS["costs_300/%s" % _c] = functools.partial(_cost_pairs, 620, 300, _c)
    PAIRS["costs_1100/%s" % _c] = functools.partial(_cost_pairs, 621, 1100, _c)
for _N in RING_N:
    PAIRS["ring_N%d" % _N] = functools.partial(_ring, _N)
PAIRS["threads_1100x8192"] = functools.partial(_wide, 630, 1100, 8192)          # all 1024 threads across a ring reload
PAIRS["waves_2100x4104"] = functools.partial(_wide, 631, 2100, 4104)            # 513 threads: 9 waves


@functools.lru_cache(maxsize=None)
def pairs(name):
    return PAIRS[name]()


@functools.lru_cache(maxsize=None)
def pair_reference(name, n, free):
    """pairwise_align_ref.align of pair n of a case (at most about 10 M cells each); shared, so do not write into it"""
    case = pairs(name)
    assert (len(case.refs[n]) + 1) * (len(case.queries[n]) + 1) <= 10500000
    return R.align(case.refs[n], case.queries[n], *case.costs, free)


# ---- closed forms, for sizes beyond the reference; tests/test_align_limits_ref.py proves each equal to the reference at small sizes
def identical_rows(n, seed=640):
    row = letters(np.random.default_rng(seed), n)
    return row, list(row)


def identical_result(n, costs):
    """a row of n random labels against itself, match > 0 and a gap dearer than nothing: n matches (either end-gap mode)"""
    return R.Result(costs[0] * n, n, 0, 0, n, np.ones(n, dtype=np.uint8))


def unequal_rows(N, M):
    """a reference of N labels 1 against a query of M labels 2: nothing matches"""
    return [1] * N, [2] * M


UNEQUAL_COSTS = (7, -1024, 1024, 1024)


def unequal_score(N, M, free):
    """N >= M, costs UNEQUAL_COSTS: a mismatch costs what one gap column does and replaces two, so M mismatches and N - M gap
    columns; with free end gaps aligning nothing (score 0) beats every column"""
    assert N >= M
    return 0 if free else -1024 * N


def unequal_free_ops(N, M):
    """with free end gaps the end cell is (N, 0): the whole reference, then the whole query, as end gaps"""
    return np.array([R.OP_REF_GAP] * N + [R.OP_QUERY_GAP] * M, dtype=np.uint8)


def equal_rows(N, M):
    return [3] * N, [3] * M


EQUAL_COSTS = (1024, -1024, 1024, 1024)


def equal_score(N, M, free):
    """N >= M, all labels equal: M matches; the N - M gap columns cost 1024 each unless they are end gaps"""
    assert N >= M
    return 1024 * M if free else 1024 * (2 * M - N)


# ========================================================================================================= the quality profile
PROFILE_CLASSES = 5


def profile_inputs(seed, M):
    """random qual (0..93) and dwell (0..50) rows for a query of M labels"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 94, size=(1, M)).astype(np.uint8), rng.integers(0, 51, size=(1, M)).astype(np.int32)


def profile_reference(ops, ref, query, qual, dwell, count_ends):
    """quality_profile_ref.profile of one pair given as an op row and two label lists"""
    ops = np.asarray(ops, dtype=np.uint8)[None]
    ref, query = np.asarray(ref, dtype=np.int32)[None], np.asarray(query, dtype=np.int32)[None]
    return PR.profile(ops, [ops.shape[1]], ref, [ref.shape[1]], query, [query.shape[1]], qual, dwell, PROFILE_CLASSES, count_ends)


@functools.lru_cache(maxsize=None)
def synthetic_ops(kind):
    """(ops, ref, query) with exactly 65535 reference and 8192 query labels, by quality_profile_cases.rows_for.  "longest": 73727
    columns, the most an op string of those rows can have -- which leaves no room for a match or a mismatch: 65535 op 3s and 8192
    op 4s, shuffled.  "mixed": 8000 columns of ops 1 / 2 among 57535 op 3s and 192 op 4s, 65727 columns"""
    rng = np.random.default_rng(650)
    N, M = LONGEST
    if kind == "longest":
        ops = np.array([3] * N + [4] * M, dtype=np.uint8)
    else:
        assert kind == "mixed"
        ops = np.array([1] * 7000 + [2] * 1000 + [3] * (N - 8000) + [4] * (M - 8000), dtype=np.uint8)
    rng.shuffle(ops)
    ref, query = PC.rows_for(rng, ops, PROFILE_CLASSES)
    assert len(ref) == N and len(query) == M
    return ops, ref, query
