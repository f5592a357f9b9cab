"""Inputs of the numeric-limit tests of the three pore-model tools (kmer_events, signal_align, signal_map), built once from seeds,
with their references cached.  Nothing here is random at test time and nothing is taken from a kernel: every expected number comes
from tests/kmer_events_ref.py, tests/signal_align_ref.py or tests/signal_map_ref.py (Python integers), or from the numpy-vectorised
table reference below, which tests/test_signal_limits_ref.py holds equal to the plain loop.  What the tools share is
csrc/wn_signal_dev.h (quantise, sa_sample_cost, sa_model_row); the sections follow its limits:

    1  the sample cost min((d d w) >> S, max_cost) + offset over a grid of model rows and samples, S and max_cost swept
    2  the quantisation at ties, at +-(2^23 - 1) and one step beyond, float32 and int16 + scale_shift
    3  event sums at their largest and negative
    4  the table kernel of kmer_events across workgroups (its launch geometry is mirrored in table_grid)
    5  the longest read of signal_map and the forced diagonal of signal_align under models of extreme cost"""
import collections
import functools

import numpy as np

from tests import kmer_events_ref as ER
from tests import signal_align_ref as AR
from tests import signal_map_ref as MR

Q_MAX = (1 << 23) - 1                   # the largest |q| and |level|
OFFSET_MAX = (1 << 30) - 1
WEIGHT_MAX = (1 << 31) - 1
COST_MAX = (1 << 31) - 1
COST_BITS = 8


def kmer_labels(code, k):
    """the k bases (1..4) of a k-mer index, first base most significant"""
    return [((code >> (2 * (k - 1 - i))) & 3) + 1 for i in range(k)]


# ---- 1. the sample cost ------------------------------------------------------------------------------------------------------------
GRID_K = 3
GRID_LEVELS = (Q_MAX, -Q_MAX, 1, -1, 0, 1234567)
GRID_WEIGHTS = (1, 2, 1 << 16, 1 << 30, WEIGHT_MAX, 3160487)
GRID_OFFSETS = (OFFSET_MAX, -OFFSET_MAX, 0)
GRID_SHIFTS = (16, 17, 31, 32, 33, 47, 48, 62, 63)
GRID_MAX_COSTS = (1, 12345, COST_MAX)
GRID_FRAC = (0, 20)


@functools.lru_cache(maxsize=None)
def grid_model():
    """[64, 3] int64: every (level, weight) pair of the grid at least once, the offsets rotating through them"""
    rows = []
    for i in range(4 ** GRID_K):
        li, wi = i % 6, (i // 6) % 6
        rows.append([GRID_LEVELS[li], GRID_WEIGHTS[wi], GRID_OFFSETS[(li + wi + i // 36) % 3]])
    return np.array(rows, dtype=np.int64)


def de_bruijn(k):
    """the linear de Bruijn sequence of order k over 1..4: 4^k + k - 1 bases, every k-mer once (the standard Lyndon-word
    construction, its first k - 1 symbols appended)"""
    n, seq, a = 4, [], [0] * (4 * k)

    def db(t, p):
        if t > k:
            if k % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, n):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return [v + 1 for v in seq + seq[:k - 1]]


@functools.lru_cache(maxsize=None)
def grid_reference():
    """66 bases with every 3-mer once, a wall, and the first ten bases again: 75 states, 64..66 walls, 67..74 repeats"""
    seq = de_bruijn(GRID_K)
    return np.array(seq + [0] + seq[:10], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def grid_q():
    """40 quantised samples: the edges and 31 seeded values over the whole range"""
    rng = np.random.default_rng(1001)
    edges = [0, 1, -1, 1 << 16, -(1 << 16), 1 << 22, -(1 << 22), Q_MAX, -Q_MAX]
    return edges + [int(v) for v in rng.integers(-Q_MAX, Q_MAX + 1, size=31)]


def grid_signal(frac_bits):
    """[40, 2] float32: x = q 2^-F, exact in float32 for |q| < 2^24; the second column lies past every read and holds a NaN"""
    x = np.array(grid_q(), dtype=np.float64) * 2.0 ** -frac_bits
    sig = np.full((len(x), 2), np.nan, dtype=np.float32)
    sig[:, 0] = x.astype(np.float32)
    assert (sig[:, 0].astype(np.float64) == x).all()
    return sig


def grid_products():
    """[40][64] Python integers: d d weight of every (sample, model row)"""
    model = grid_model().tolist()
    return [[(q - level) ** 2 * weight for level, weight, _ in model] for q in grid_q()]


@functools.lru_cache(maxsize=None)
def grid_costs(S, max_cost):
    """[40][64] Python integers: signal_align_ref.sample_cost of every sample against every model row"""
    model = grid_model().tolist()
    return [[AR.sample_cost(q, level, weight, offset, S, max_cost) for level, weight, offset in model] for q in grid_q()]


@functools.lru_cache(maxsize=None)
def grid_map_reference(frac_bits, S, max_cost):
    sig = grid_signal(frac_bits)
    return MR.signal_map_ref(sig, np.ones(len(sig), dtype=np.int32), grid_reference(), grid_model(), GRID_K, frac_bits=frac_bits,
                             weight_shift=S, max_cost=max_cost)


@functools.lru_cache(maxsize=None)
def grid_align_inputs(frac_bits):
    """every (sample, k-mer) pair as a read of its own with T = N = 1: signal [2560, 2], labels [2560, 3]; read 64 s + c is sample s
    in k-mer c"""
    sig = grid_signal(frac_bits)
    n = 4 ** GRID_K
    labels = np.array([kmer_labels(c, GRID_K) for c in range(n)], dtype=np.int32)
    return np.repeat(sig, n, axis=0), np.tile(labels, (len(sig), 1))


# ---- 2. quantisation ---------------------------------------------------------------------------------------------------------------
QUANT_FRAC = (0, 1, 12, 20)
# in units of q (x = value 2^-F, exact in float32): ties both ways near 0, ties at 23 and 24 significant bits, the neighbours of a
# tie, -0.0, and the two ends of the range; the denormal is appended as it is
QUANT_VALUES = (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 4194304.5, 4194305.5, -4194304.5, 8388606.5, -8388606.5, 0.75, 0.25, -0.75, 3.0,
                -0.0, float(Q_MAX), float(-Q_MAX), 8388606.0, 1000001.5)
QUANT_DENORMAL = float(np.float32(1e-40))
# each makes its read bad: the first value out of range on each sign, and the tie that rounds (to even) onto it
QUANT_BEYOND = (8388608.0, -8388608.0, 8388607.5)
QUANT_BAD_READS = (1, 3, 4)

QuantCase = collections.namedtuple("QuantCase", "signal signal_lengths scale_shift frac_bits labels label_lengths starts")


def _one_sample_events(signal, scale_shift, frac_bits):
    B, n = signal.shape
    return QuantCase(signal, np.full(B, n, dtype=np.int32), scale_shift, frac_bits, np.ones((B, n), dtype=np.int32),
                     np.full(B, n, dtype=np.int32), np.tile(np.arange(n + 1, dtype=np.int32), (B, 1)))


@functools.lru_cache(maxsize=None)
def quant_f32_case(frac_bits):
    """six reads of 21 one-sample events: good, bad (+2^23 among the values), good (reversed), bad (-2^23), bad (the tie), good"""
    scale = 2.0 ** -frac_bits
    good = np.array([v * scale for v in QUANT_VALUES] + [QUANT_DENORMAL], dtype=np.float64)
    assert (good.astype(np.float32).astype(np.float64) == good).all()              # every value is a float32
    rows = [good, good.copy(), good[::-1].copy(), good.copy(), good.copy(), good.copy()]
    for b, v, at in zip(QUANT_BAD_READS, QUANT_BEYOND, (7, 0, 20)):
        rows[b][at] = v * scale
    return _one_sample_events(np.array(rows, dtype=np.float32), None, frac_bits)


QUANT_I16_FRAC = 12
# (raw samples, scale, shift) per read at F = 12, where |v| must stay below 2048.  Scales 0.5 and float32(0.1) carry the extreme
# raw values out of range (32767 / 2 = 16383.5), so those two reads hold the largest raw values that stay inside instead; their
# shifts put v 2^12 of a small raw value so close to a tie that evaluating x scale + shift in float32 rounds the other way.  The
# reads at scale 2^-4 hold the extreme raw values: 32767 * 256 + 255 = 2^23 - 1 exactly, and -32768 * 256 + 1 = -(2^23 - 1).
_SMALL = (-1, 1, 3)
QUANT_I16_READS = (
    ((-4095,) + _SMALL + (4095,), 0.5, 2.0 ** -13 * (1.0 + 2.0 ** -20)),
    ((-20400,) + _SMALL + (20400,), float(np.float32(0.1)), 1.9550049304962158),
    ((-32768,) + _SMALL + (32767,), 0.0625, 255.0 / 4096.0),                       # lands on 2^23 - 1
    ((-32768,) + _SMALL + (32767,), 0.0625, 1.0 / 4096.0),                         # lands on -(2^23 - 1)
    ((-32768,) + _SMALL + (32767,), 0.0625, 256.0 / 4096.0),                       # bad: 2^23
    ((-32768,) + _SMALL + (32767,), 0.0625, 0.0),                                  # bad: -2^23
    ((-32768,) + _SMALL + (32767,), float(np.nextafter(np.float32(0.0625), np.float32(1.0))), 255.0 / 4096.0),   # bad: the next scale
    ((-4095,) + _SMALL + (4095,), 0.5, 0.0),
)
QUANT_I16_BAD_READS = (4, 5, 6)


@functools.lru_cache(maxsize=None)
def quant_i16_case():
    raw = np.array([r[0] for r in QUANT_I16_READS], dtype=np.int16)
    ss = np.array([[r[1], r[2]] for r in QUANT_I16_READS], dtype=np.float32)
    assert (ss.astype(np.float64) == np.array([[r[1], r[2]] for r in QUANT_I16_READS])).all()      # every pair is float32
    return _one_sample_events(raw, ss, QUANT_I16_FRAC)


def quantise_in_float32(raw, scale, shift, frac_bits):
    """what a kernel would get that formed x scale + shift in float32 (two roundings, or one with an fma): for the precondition"""
    two = np.float32(np.float32(raw) * np.float32(scale)) + np.float32(shift)
    fma = np.float32(float(raw) * float(scale) + float(shift))
    return round(float(two) * (1 << frac_bits)), round(float(fma) * (1 << frac_bits))


def quant_events_reference(case):
    return ER.kmer_events_ref(case.signal, case.signal_lengths, case.labels, case.label_lengths, case.starts[:, :-1], case.starts[:, 1:],
                              case.label_lengths, k=1, first=0, scale_shift=case.scale_shift, frac_bits=case.frac_bits)


def quant_expected_q(case):
    """[B][n]: the reference's q of every sample, None where it is not finite or out of range"""
    ss = case.scale_shift
    return [[ER.quantise(x, None if ss is None else ss[b], case.frac_bits) for x in row.tolist()] for b, row in enumerate(case.signal)]


QUANT_K = 3


def quant_model(cases):
    """[64, 3] int64 for the cases' samples seen through signal_map and signal_align: weight 2^16 at S = 16, offset 0, so a sample
    costs min((q - level)^2, 2^31 - 1).  Row 0 has level 0 (cost q^2); the others take the expected q of the cases in turn and
    then their successors, so that every sample meets a row it costs 0 in and a q that is off by one shows as a cost of 1"""
    want = sorted({q for case in cases for row in quant_expected_q(case) for q in row if q is not None} - {0})
    levels = [0] + want + [q + 1 for q in want if q + 1 not in want and q + 1 < Q_MAX]
    assert len(want) < 4 ** QUANT_K
    levels = (levels + [0] * 64)[:4 ** QUANT_K]
    return np.array([[level, 1 << 16, 0] for level in levels], dtype=np.int64)


def quant_samples_as_reads(case):
    """every sample as a read of its own: (signal [B n, 1], scale_shift [B n, 2] or None)"""
    B, n = case.signal.shape
    ss = None if case.scale_shift is None else np.repeat(case.scale_shift, n, axis=0)
    return case.signal.reshape(B * n, 1).copy(), ss


def quant_costs(case, model):
    """[B n][64] Python integers, or None for a sample that makes its read bad"""
    rows = model.tolist()
    return [None if q is None else [AR.sample_cost(q, level, weight, offset, 16, COST_MAX) for level, weight, offset in rows]
            for read in quant_expected_q(case) for q in read]


# ---- 3. the largest event sums -----------------------------------------------------------------------------------------------------
BIG_EVENTS = (65536, 65536, 33, 32, 1)
BIG_BASE = 3
BIG_KW = dict(k=1, first=0, frac_bits=0)


@functools.lru_cache(maxsize=None)
def big_case():
    """two reads of five events, every sample -(2^23 - 1) in read 0 and +(2^23 - 1) in read 1; all labels the same base"""
    n = len(BIG_EVENTS)
    starts = np.tile(np.concatenate([[0], np.cumsum(BIG_EVENTS)]).astype(np.int32), (2, 1))
    T = int(starts[0, -1])
    signal = np.empty((2, T), dtype=np.float32)
    signal[0], signal[1] = -float(Q_MAX), float(Q_MAX)
    return QuantCase(signal, np.full(2, T, dtype=np.int32), None, 0, np.full((2, n), BIG_BASE, dtype=np.int32),
                     np.full(2, n, dtype=np.int32), starts)


def big_rows(reads):
    c = big_case()
    return QuantCase(c.signal[reads], c.signal_lengths[reads], None, 0, c.labels[reads], c.label_lengths[reads], c.starts[reads])


@functools.lru_cache(maxsize=None)
def big_reference(reads=(0, 1), max_dwell=255, twice=False):
    """the plain-loop reference of the reads; twice: the same batch added a second time into the first one's tables"""
    case = big_rows(list(reads))
    args = (case.signal, case.signal_lengths, case.labels, case.label_lengths, case.starts[:, :-1], case.starts[:, 1:], case.label_lengths)
    out = ER.kmer_events_ref(*args, max_dwell=max_dwell, **BIG_KW)
    if twice:
        out = ER.kmer_events_ref(*args, max_dwell=max_dwell, tables=out["tables"], **BIG_KW)
    return out


# ---- 4. the table kernel across workgroups -----------------------------------------------------------------------------------------
TABLE_CHUNK, TABLE_BLOCKS, TABLE_THREADS = 4096, 256, 256          # csrc/wn_events.hip: kEvTableChunk, kEvTableBlocks, kEvThreads


def table_grid(rows):
    """(workgroups, chunk) of kmer_tables_kernel for `rows` = B N flattened events, as wn_kmer_events computes them"""
    blocks = min(max((rows + TABLE_CHUNK - 1) // TABLE_CHUNK, 1), TABLE_BLOCKS)
    per = (rows + blocks - 1) // blocks
    return blocks, (per + TABLE_THREADS - 1) // TABLE_THREADS * TABLE_THREADS


TableCase = collections.namedtuple("TableCase", "signal signal_lengths labels label_lengths starts bad_reads")


def _table_case(seed, B, N, dwell_hi, faults):
    """B reads of N events of 1 .. dwell_hi - 1 samples, labels N + 4 wide; faults: {read: "nan" | "label" | "length"}"""
    rng = np.random.default_rng(seed)
    dwell = rng.integers(1, dwell_hi, size=(B, N)) if dwell_hi > 2 else np.ones((B, N), dtype=np.int64)
    starts = np.concatenate([np.zeros((B, 1), dtype=np.int64), np.cumsum(dwell, axis=1)], axis=1).astype(np.int32)
    L = int(starts[:, -1].max())
    signal = (90.0 + 12.0 * rng.standard_normal((B, L))).astype(np.float32)
    labels = rng.integers(1, 5, size=(B, N + 4)).astype(np.int32)
    sl, ll = starts[:, -1].copy(), np.full(B, N + 4, dtype=np.int32)
    for b, what in faults.items():
        if what == "nan":
            signal[b, starts[b, N // 2]] = np.nan                    # the first sample of event N / 2, used under every window
        elif what == "label":
            labels[b, N // 3] = 0
        else:
            sl[b] = -1
    return TableCase(signal, sl, labels, ll, starts, tuple(sorted(faults)))


@functools.lru_cache(maxsize=None)
def table_case(name):
    """three: 37 x 300 events of 1..3 samples, three workgroups, reads 12 and 25 across the seams, 12 and 30 bad
    cap: 2050 x 513 one-sample events, more than 256 x 4096 rows, bad reads on the seams of workgroups 1, 100 and 241 and at the end
    cap_small: the cap's construction at 40 x 513, small enough for the plain loop"""
    if name == "three":
        return _table_case(401, 37, 300, 4, {12: "nan", 30: "length"})
    if name == "cap":
        chunk = table_grid(2050 * 513)[1]
        return _table_case(402, 2050, 513, 2, {chunk // 513: "nan", 100 * chunk // 513: "label", 241 * chunk // 513: "length", 2049: "nan"})
    assert name == "cap_small"
    return _table_case(403, 40, 513, 2, {8: "nan", 17: "label", 33: "length", 39: "nan"})


TABLE_WINDOWS = {1: 0, 2: 0, 6: -2}                                 # k: first


def fast_events_ref(signal, signal_lengths, labels, label_lengths, begin, end, events, k, first, frac_bits=12, max_dwell=255,
                    scale_shift=None):
    """kmer_events_ref (frame_stride 1, frame_offset 0) in whole-array numpy: the same dict without "tables".  int64 throughout:
    for signals whose sums of q^2 over a read stay below 2^63.  Held equal to the plain loop by tests/test_signal_limits_ref.py."""
    B, N = begin.shape
    L, n_lab = signal.shape[1], labels.shape[1]
    sl, ll, ne = (np.asarray(a, dtype=np.int64) for a in (signal_lengths, label_lengths, events))
    bg, en = begin.astype(np.int64), end.astype(np.int64)
    j = np.arange(N, dtype=np.int64)[None, :]
    bad = ~((sl >= 0) & (sl <= L) & (ll >= 0) & (ll <= n_lab) & (ne >= 0) & (ne <= N))
    live = (j < ne[:, None]) & ~bad[:, None]
    prev_end = np.concatenate([np.zeros((B, 1), dtype=np.int64), en[:, :-1]], axis=1)
    bad |= (live & ((bg < 0) | (en < bg) | ((j > 0) & (bg < prev_end)))).any(axis=1)
    live &= ~bad[:, None]
    slc = np.clip(sl, 0, L)[:, None]
    c0, c1 = np.minimum(np.maximum(bg, 0), slc), np.minimum(np.maximum(en, 0), slc)
    length = c1 - c0
    w0 = j + first
    code = np.where(length == 0, -2, np.where((en > slc) | (length > ER.MAX_EVENT), -3, np.where((w0 < 0) | (w0 + k > ll[:, None]), -1, 0)))
    used = live & (code == 0)
    rows = np.arange(B)[:, None]
    idx = np.zeros((B, N), dtype=np.int64)
    for i in range(k):
        lab = labels[rows, np.clip(w0 + i, 0, n_lab - 1)].astype(np.int64)
        bad |= (used & ((lab < 1) | (lab > 4))).any(axis=1)
        idx = idx * 4 + ((lab - 1) & 3)
    v = signal.astype(np.float64)
    if scale_shift is not None:
        v = v * scale_shift[:, :1].astype(np.float64) + scale_shift[:, 1:].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(v * float(1 << frac_bits))
        fine = np.isfinite(r) & (np.abs(r) < ER.Q_LIMIT)
    q = np.where(fine, r, 0.0).astype(np.int64)
    zero = np.zeros((B, 1), dtype=np.int64)
    cum_bad = np.concatenate([zero, np.cumsum(~fine, axis=1)], axis=1)
    cum_q = np.concatenate([zero, np.cumsum(q, axis=1)], axis=1)
    cum_q2 = np.concatenate([zero, np.cumsum(q * q, axis=1)], axis=1)
    bad |= (used & (cum_bad[rows, c1] != cum_bad[rows, c0])).any(axis=1)
    live &= ~bad[:, None]
    used &= live
    kmer = np.where(live, np.where(used, idx, code), -4).astype(np.int32)
    start = np.where(live, c0, 0).astype(np.int32)
    length = np.where(live, length, 0).astype(np.int32)
    total = np.where(used, cum_q[rows, c1] - cum_q[rows, c0], 0)
    squares = np.where(used, cum_q2[rows, c1] - cum_q2[rows, c0], 0)
    counts = np.stack([used.sum(1), (live & (kmer == -1)).sum(1), (live & ((kmer == -2) | (kmer == -3))).sum(1), (length * used).sum(1)], axis=1)
    counts[bad] = -1
    n_codes = 4 ** k
    codes = kmer[used].astype(np.int64)
    stats = np.zeros((n_codes, 5), dtype=np.int64)
    for col, values in enumerate((np.ones_like(codes), length[used].astype(np.int64), total[used], squares[used] & 0xffffffff, squares[used] >> 32)):
        np.add.at(stats[:, col], codes, values)
    hist = np.bincount(codes * (max_dwell + 1) + np.minimum(length[used], max_dwell), minlength=n_codes * (max_dwell + 1))
    return {"kmer": kmer, "start": start, "length": length, "sum": total, "sumsq": squares, "read_counts": counts.astype(np.int32),
            "kmer_stats": stats, "dwell_hist": hist.reshape(n_codes, max_dwell + 1).astype(np.int64), "bad": int(bad.sum())}


def _table_args(case):
    B, N = case.starts.shape[0], case.starts.shape[1] - 1
    return (case.signal, case.signal_lengths, case.labels, case.label_lengths, case.starts[:, :-1], case.starts[:, 1:],
            np.full(B, N, dtype=np.int32))


@functools.lru_cache(maxsize=None)
def table_reference(name, k):
    """the vectorised reference of a table case at k (first = TABLE_WINDOWS[k]), F = 12, max_dwell 255"""
    return fast_events_ref(*_table_args(table_case(name)), k=k, first=TABLE_WINDOWS[k])


@functools.lru_cache(maxsize=None)
def table_plain_reference(name, k):
    return ER.kmer_events_ref(*_table_args(table_case(name)), k=k, first=TABLE_WINDOWS[k], frac_bits=12, max_dwell=255)


# ---- 5. long paths -----------------------------------------------------------------------------------------------------------------
PATH_K = 2
MAP_T = 4096                            # mapping.MAX_MAP_SIGNAL: the whole dynamic LDS of signal_map_kernel
MAP_M = 5200
MAP_LENGTHS = (4096, 4095, 1, 1)
MAP_STRIPS = (64, 2048, None)

PathModel = collections.namedtuple("PathModel", "model weight_shift max_cost draw")


@functools.lru_cache(maxsize=None)
def path_model(which):
    """costly: weight 2^31 - 1 at S = 16 clamped at 2^31 - 1, offsets at 2^30 - 1 and just below, levels within 1000 of 2^23 - 1 and
    samples within 1000 of -(2^23 - 1): nearly every cell costs 2^31 - 1 + offset, the largest a cell can cost; one sample in twelve
    sits within 3 of a level instead, where the quadratic term is below the clamp, so the path depends on the samples.
    cheap: levels 1000 + 40 i in a seeded order, weight 2^16 at S = 16 (cost d^2), offsets at -(2^30 - 1) and just above; a sample
    lies within 3 of a level: a cell costs little more than -(2^30 - 1), the least a cell can cost.  draw(rng, n) gives n quantised
    samples (F = 0)."""
    rng = np.random.default_rng(501 if which == "costly" else 502)
    n = 4 ** PATH_K
    if which == "costly":
        levels = Q_MAX - rng.integers(0, 1000, size=n)
        model = np.stack([levels, np.full(n, WEIGHT_MAX), OFFSET_MAX - rng.integers(0, 6, size=n)], axis=1).astype(np.int64)

        def draw(r, count):
            q = -Q_MAX + r.integers(0, 1000, size=count)
            near = r.random(count) < 1.0 / 12.0
            return np.where(near, levels[r.integers(0, n, size=count)] - r.integers(0, 4, size=count), q)
    else:
        levels = 1000 + 40 * rng.permutation(n)
        model = np.stack([levels, np.full(n, 1 << 16), -OFFSET_MAX + rng.integers(0, 6, size=n)], axis=1).astype(np.int64)

        def draw(r, count):
            return levels[r.integers(0, n, size=count)] + r.integers(-3, 4, size=count)
    return PathModel(model, 16, COST_MAX, draw)


MapCase = collections.namedtuple("MapCase", "signal signal_lengths ref model kw")


@functools.lru_cache(maxsize=None)
def map_long_case(which):
    """L = 4096 exactly, reads of 4096, 4095, 1 and 1 samples, 5200 states (two walls among them) under a path model.  Under the
    cheap model the two long reads follow the reference from states 1600 and 3400, stepping at two samples in five, so that the
    best path is a long walk between the walls and not a stay"""
    pm = path_model(which)
    rng = np.random.default_rng(511 if which == "costly" else 512)
    ref = rng.integers(1, 5, size=MAP_M + PATH_K - 1).astype(np.int32)
    ref[1500] = ref[3333] = 0
    signal = np.stack([pm.draw(rng, MAP_T) for _ in MAP_LENGTHS]).astype(np.float32)
    kw = dict(k=PATH_K, frac_bits=0, weight_shift=pm.weight_shift, max_cost=pm.max_cost)
    if which == "cheap":
        codes, _ = MR.prepare(ref, pm.model, PATH_K)
        for b, s0 in enumerate((1600, 3400)):
            states = s0 + np.cumsum(rng.random(MAP_T) < 0.4)
            assert states[-1] < MAP_M and (codes[states] >= 0).all()
            signal[b] = pm.model[codes[states], 0] + rng.integers(-3, 4, size=MAP_T)
    return MapCase(signal, np.array(MAP_LENGTHS, dtype=np.int32), ref, pm.model, kw)


@functools.lru_cache(maxsize=None)
def map_long_reference(which):
    case = map_long_case(which)
    return MR.signal_map_ref(case.signal, case.signal_lengths, case.ref, case.model, **case.kw)


AlignCase = collections.namedtuple("AlignCase", "signal signal_lengths labels label_lengths model kw")
DIAGONAL = {64: ((65, 65), (320, 320), (321, 321), (577, 577), (66, 65), (321, 320), (322, 321), (578, 577)),
            512: ((600, 600), (601, 600))}                          # band: (T, N) per read


@functools.lru_cache(maxsize=None)
def diagonal_case(which, band):
    pm = path_model(which)
    rng = np.random.default_rng(520 + band + (which == "costly"))
    shapes = DIAGONAL[band]
    B, L, n_lab = len(shapes), max(t for t, _ in shapes), max(n for _, n in shapes) + PATH_K - 1
    signal = np.stack([pm.draw(rng, L) for _ in shapes]).astype(np.float32)
    labels = rng.integers(1, 5, size=(B, n_lab)).astype(np.int32)
    kw = dict(k=PATH_K, first=0, band=band, frac_bits=0, weight_shift=pm.weight_shift, max_cost=pm.max_cost)
    if which == "cheap":                                             # sample t within 3 of the level of state min(t, N - 1)
        for b, (t, n) in enumerate(shapes):
            codes = np.array(AR.read_states(labels[b], n + PATH_K - 1, PATH_K, 0))
            signal[b, :t] = pm.model[codes[np.minimum(np.arange(t), n - 1)], 0] + rng.integers(-3, 4, size=t)
    return AlignCase(signal, np.array([t for t, _ in shapes], dtype=np.int32), labels,
                     np.array([n + PATH_K - 1 for _, n in shapes], dtype=np.int32), pm.model, kw)


@functools.lru_cache(maxsize=None)
def diagonal_reference(which, band):
    case = diagonal_case(which, band)
    return AR.signal_align_ref(case.signal, case.signal_lengths, case.labels, case.label_lengths, case.model, **case.kw)


def diagonal_sum(case, b):
    """the cost of read b along the diagonal (state t at sample t), sample by sample in Python integers; T = N only"""
    T = int(case.signal_lengths[b])
    codes = AR.read_states(case.labels[b], int(case.label_lengths[b]), PATH_K, 0)
    assert len(codes) == T
    rows = case.model.tolist()
    return sum(AR.sample_cost(int(case.signal[b, t]), *rows[codes[t]], case.kw["weight_shift"], case.kw["max_cost"]) for t in range(T))
