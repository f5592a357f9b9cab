"""The inputs that tests/test_pileup_limits_ref.py (CPU) and tests/test_gpu_pileup_limits.py share, each built once from fixed
seeds or by construction: the pileup kernel at its wave and tile seams, at whole tiles and waves of one op, at its size and batch
limits; the consensus scan beyond one tile total per thread; the calling rules beside 2^31; and a pile with every kind of record.
T = 256 op columns is the pileup kernel's tile, a wave is 64 of them.

Everything here is a CONDITION, not a measurement: tests/test_pileup_limits_ref.py proves from tests/pileup_ref.py alone what
each case reaches, so that the GPU file cannot pass vacuously."""
import functools
from collections import namedtuple

import numpy as np

from tests import pileup_ref as P

T = 256
WAVE = 64
MAX_REF, MAX_QUERY = 65535, 8192
MAX_OPS = MAX_REF + MAX_QUERY
MAX_BATCH = 65535
SEAMS = tuple(range(WAVE, 2 * T + 1, WAVE))
PAD = 7                                       # the byte past ops_len: no op

Reads = namedtuple("Reads", "ops ops_len lo n_ref strand query query_len R max_ins keep")
Rows = namedtuple("Rows", "pile ref")         # a hand-made P.Pile and its reference labels


def _count(string, skip):
    return int(np.count_nonzero(np.asarray(string, dtype=np.uint8) != skip))


def pack(strings, queries, lo, strand, max_ins, R=None, keep=None, width=None, query_width=None, n_ref=None):
    """Reads of op strings and label lists: rows padded with PAD (ops) and 0 (labels), the lengths from the strings themselves"""
    B = len(strings)
    ops = np.full((B, max(1, max(len(s) for s in strings)) if width is None else width), PAD, dtype=np.uint8)
    query = np.zeros((B, max(1, max(len(q) for q in queries)) if query_width is None else query_width), dtype=np.int32)
    for b, (s, q) in enumerate(zip(strings, queries)):
        ops[b, :len(s)] = s
        query[b, :len(q)] = q
    n_ref = [_count(s, 4) for s in strings] if n_ref is None else n_ref
    R = max(a + n for a, n in zip(lo, n_ref)) if R is None else R
    i32 = lambda v: np.asarray(v, dtype=np.int32)                    # noqa: E731
    return Reads(ops, i32([len(s) for s in strings]), i32(lo), i32(n_ref), i32(strand), query, i32([len(q) for q in queries]), int(R), max_ins,
                 None if keep is None else np.asarray(keep, dtype=bool))


def on_strand(reads, strand):
    """the same reads, all on one strand: a reverse-strand read walks the same columns back to front"""
    return reads._replace(strand=np.full_like(reads.strand, strand))


def reference_pile(reads, into=None):
    return P.pileup_ref(reads.ops, reads.ops_len, reads.lo, reads.n_ref, reads.strand, reads.query, reads.query_len, reads.R,
                        max_ins=reads.max_ins, keep=reads.keep, into=into)


def _labels(rng, n, odd=0.1):
    """n random labels, a share `odd` of them outside 1..4"""
    v = rng.integers(1, 5, size=n)
    return [int(x) for x in np.where(rng.random(n) < odd, rng.choice([0, 5, 9], size=n), v)]


# ---- the seam grid --------------------------------------------------------------------------------------------------------------

GRID_MAX_INS = 4
GRID_OFFSETS = range(0, 2 * T + 9)
GRID_SHIFTED = ("run3", "run_max", "run_over")                       # the variants whose labels follow the reference index
GRID_VARIANTS = GRID_SHIFTED + ("ends", "first", "last")
GRID_REF = 2 * T + 20                                                # reference labels of a shifted read, whatever its offset
MOTIF = [1, 4, 4, 4, 1, 3, 4, 2]              # a run of 3, a deletion, and a run of 1 ended by an aligned column
MOTIF_RUN = [1, 4, 9, 3, 2]                   # labels of the run (slot 2 is no base and stays uncounted)
MOTIF_ALIGNED = [2, 3, 5]                     # labels of the three aligned columns (the last one is `other`)
MOTIF_SINGLE = 4                              # the run of 1


def motif(run):
    return [1] + [4] * run + MOTIF[4:]


def _ends(n, ref_first=True):
    """n end columns: reference labels against gaps and query labels against gaps"""
    a, b = [3] * (n // 2), [4] * (n - n // 2)
    return a + b if ref_first else b + a


def grid_string(variant, s):
    tail = [1] * (2 * T + 16 - s)
    if variant in GRID_SHIFTED:
        return [1] * s + motif({"run3": 3, "run_max": GRID_MAX_INS, "run_over": GRID_MAX_INS + 1}[variant]) + tail
    if variant == "ends":                                            # end columns in front: the first aligned column is not column 0
        return [3] * 5 + [4] * 3 + [1] * s + MOTIF + tail
    if variant == "first":                                           # the first aligned column sits exactly at s
        return _ends(s) + MOTIF + tail
    head = [1] * (s - 7) + MOTIF if s >= 7 else [1] * (s + 1)        # "last": the last aligned column sits exactly at s
    return head + _ends(2 * T + 16 - s, ref_first=False)


@functools.lru_cache(maxsize=None)
def grid_reference_labels():
    """the label a shifted read shows at reference index i outside its motif"""
    return tuple(_labels(np.random.default_rng(101), GRID_REF))


def shifted_query(variant, s):
    """labels of a GRID_SHIFTED read: the motif's own inside it, grid_reference_labels() by reference index outside"""
    G = grid_reference_labels()
    run = len(grid_string(variant, s)) - (2 * T + 16) - 5
    inside = [MOTIF_ALIGNED[0]] + MOTIF_RUN[:run] + [MOTIF_ALIGNED[1], MOTIF_SINGLE, MOTIF_ALIGNED[2]]
    return list(G[:s]) + inside + list(G[s + 4:])


@functools.lru_cache(maxsize=None)
def grid():
    """Reads on strand 0 (use on_strand): every variant at every offset, windows at lo = b % 5"""
    rng = np.random.default_rng(102)
    strings, queries = [], []
    for variant in GRID_VARIANTS:
        for s in GRID_OFFSETS:
            strings.append(grid_string(variant, s))
            queries.append(shifted_query(variant, s) if variant in GRID_SHIFTED else _labels(rng, _count(strings[-1], 3)))
    B = len(strings)
    return pack(strings, queries, [b % 5 for b in range(B)], [0] * B, GRID_MAX_INS)


@functools.lru_cache(maxsize=None)
def grid_pile(strand):
    return reference_pile(on_strand(grid(), strand))


# ---- whole tiles and waves of one op --------------------------------------------------------------------------------------------

WHOLE_MAX_INS = 4
WHOLE_STRINGS = ([1] * 5 + [4] * (3 * T + 10) + [1] * 7,             # an insertion run over whole tiles, both walk directions
                 [2] * 5 + [3] * (3 * T + 10) + [2] * 7,             # a deletion run of the same length
                 [1] * 64 + [4] * 64 + [1] * 128,                    # op 4 in exactly one wave: columns 64..127, walked back 128..191
                 [1] * 192 + [4] * 64 + [1] * 64,                    # columns 192..255, walked back 64..127
                 [1] + [4] * (MAX_QUERY - 2) + [1])                  # the longest run the limits allow: 8190 columns, 30 whole tiles


@functools.lru_cache(maxsize=None)
def whole():
    rng = np.random.default_rng(103)
    queries = [_labels(rng, _count(s, 3)) for s in WHOLE_STRINGS]
    B = len(WHOLE_STRINGS)
    return pack(list(WHOLE_STRINGS), queries, [3 * b for b in range(B)], [0] * B, WHOLE_MAX_INS, query_width=MAX_QUERY)


@functools.lru_cache(maxsize=None)
def whole_pile(strand):
    return reference_pile(on_strand(whole(), strand))


# ---- the size limits ------------------------------------------------------------------------------------------------------------

SIZE_MAX_INS = 8
SIZE_STRINGS = ([2] + [3] * (MAX_REF - 2) + [4] * (MAX_QUERY - 2) + [1],           # 73725 columns: the most two aligned columns allow
                ([2] + [3] * 7) * (MAX_QUERY - 1) + [3] * 6 + [1])                # an aligned column in every tile; i to 65534, j to 8191
SIZE_R = MAX_REF + 5


@functools.lru_cache(maxsize=None)
def size():
    """both strings on both strands; lo + n_ref == R for the first of each pair, lo == 0 for the other"""
    rng = np.random.default_rng(104)
    queries = [_labels(rng, MAX_QUERY) for _ in SIZE_STRINGS]
    strings = [SIZE_STRINGS[0], SIZE_STRINGS[0], SIZE_STRINGS[1], SIZE_STRINGS[1]]
    return pack(strings, [queries[0], queries[0], queries[1], queries[1]], [SIZE_R - MAX_REF, 0, 0, SIZE_R - MAX_REF], [0, 1, 1, 0],
                SIZE_MAX_INS, R=SIZE_R, width=MAX_OPS, query_width=MAX_QUERY)


@functools.lru_cache(maxsize=None)
def size_pile():
    return reference_pile(size())


# ---- the batch limit ------------------------------------------------------------------------------------------------------------

BATCH_SKIPPED = (0, 1, 4097, 40000, MAX_BATCH - 1)                   # keep false
BATCH_BAD = (2, 3, 255, 256, 32768, MAX_BATCH - 2, MAX_BATCH - 3)    # op 0


@functools.lru_cache(maxsize=None)
def batch():
    """65535 one-column reads on R = 2, alternating strands and positions"""
    rng = np.random.default_rng(105)
    b = np.arange(MAX_BATCH)
    ops = np.ones((MAX_BATCH, 1), dtype=np.uint8)
    ops[list(BATCH_BAD)] = 0
    keep = np.ones(MAX_BATCH, dtype=bool)
    keep[list(BATCH_SKIPPED)] = False
    one = np.ones(MAX_BATCH, dtype=np.int32)
    query = np.asarray(_labels(rng, MAX_BATCH, odd=0.02), dtype=np.int32).reshape(MAX_BATCH, 1)
    return Reads(ops, one, ((b >> 1) & 1).astype(np.int32), one, (b & 1).astype(np.int32), query, one, 2, 1, keep)


@functools.lru_cache(maxsize=None)
def batch_pile():
    return reference_pile(batch())


# ---- the scan of the tile totals ------------------------------------------------------------------------------------------------

SCAN_MAX_INS = 8
SCAN_R = (T * T + 1, T * 513 - 3)             # 257 tiles: two per thread, thread 128 owns one, the rest none; 513 tiles: three per thread
SCAN_DELETED_TILE, SCAN_FULL_TILE, SCAN_BREAK_TILE = 3, 4, 200
SCAN_RULES = dict(min_depth=3, num=1, den=2)


def random_pile(rng, R, max_ins, top=4):
    counts = rng.integers(0, top, size=(R, 2, 6))
    ins_lengths = rng.integers(0, top, size=(R, max_ins + 1)) * (rng.random((R, 1)) < 0.5)
    ins_bases = rng.integers(0, 3, size=(R, max_ins, 4)) * (rng.random((R, max_ins, 1)) < 0.7)
    return P.Pile(counts.astype(np.int64), ins_lengths.astype(np.int64), ins_bases.astype(np.int64), None, 0)


@functools.lru_cache(maxsize=None)
def scan(R):
    """Rows: a random small-count pile; one tile deleted whole, one tile that emits 9 labels per position, one tile of reference
    breaks (label 0) without depth"""
    rng = np.random.default_rng(R)
    pile, ref = random_pile(rng, R, SCAN_MAX_INS), rng.integers(0, 6, size=R)
    tile = lambda t: slice(t * T, (t + 1) * T)                       # noqa: E731
    for t in (SCAN_DELETED_TILE, SCAN_FULL_TILE, SCAN_BREAK_TILE):
        pile.counts[tile(t)] = 0
        pile.ins_lengths[tile(t)] = 0
    pile.counts[tile(SCAN_DELETED_TILE), 0, P.DEL] = 3
    pile.counts[tile(SCAN_FULL_TILE), 1, 0] = 5
    pile.ins_lengths[tile(SCAN_FULL_TILE), SCAN_MAX_INS] = 6
    for k in range(SCAN_MAX_INS):
        pile.ins_bases[tile(SCAN_FULL_TILE), k, k % 4] = 3
    ref[tile(SCAN_BREAK_TILE)] = 0
    return Rows(pile, ref)


@functools.lru_cache(maxsize=None)
def scan_calls(R):
    rows = scan(R)
    return P.call_consensus_ref(rows.pile, rows.ref, **SCAN_RULES)


# ---- counts beside 2^31 ---------------------------------------------------------------------------------------------------------

TOP = 2 ** 31 - 1
DEN = 2 ** 15
NUM = DEN - 1
K = 65535                                     # c = NUM * K against d = DEN * K: c * DEN == NUM * d, both below 2^31
NUM2, K2 = DEN - 2, 81921                     # (2^14 - 1) * K2 against 2^14 * K2: equality under NUM2 / DEN, and c * DEN is 2^31 - 2^15 mod 2^32
COUNT_MAX_INS = 2
COUNT_RULES = ((3, NUM, DEN), (3, NUM2, DEN), (3, DEN, DEN), (3, 0, 1), (TOP, NUM, DEN), (TOP, 1, 2))
# name, rule ("base" or "ins"), the count c (of the candidate G, or n in one ins_lengths column), the depth d, (num, den) and
# the stated difference c * den - num * d
COUNT_PAIRS = (("base_equal", "base", NUM * K, DEN * K, (NUM, DEN), 0), ("base_called", "base", NUM * K + 1, DEN * K, (NUM, DEN), DEN),
               ("ins_equal", "ins", NUM * K, DEN * K, (NUM, DEN), 0), ("ins_called", "ins", NUM * K + 1, DEN * K, (NUM, DEN), DEN),
               ("base_equal_2", "base", (NUM2 // 2) * K2, (DEN // 2) * K2, (NUM2, DEN), 0),
               ("base_called_2", "base", (NUM2 // 2) * K2 + 1, (DEN // 2) * K2, (NUM2, DEN), DEN),
               ("ins_equal_2", "ins", (NUM2 // 2) * K2, (DEN // 2) * K2, (NUM2, DEN), 0),
               ("ins_called_2", "ins", (NUM2 // 2) * K2 + 1, (DEN // 2) * K2, (NUM2, DEN), DEN))
COUNT_NAMES = tuple(p[0] for p in COUNT_PAIRS) + ("deletion_called", "depth_below", "depth_at", "strand_split")
SPLIT = (2 ** 30 + 5, 2 ** 30 - 6)


@functools.lru_cache(maxsize=None)
def count_rows():
    """Rows in the order of COUNT_NAMES.  The reference base is A (1) where the candidate is G, so that a call shows as a flag."""
    counts, lengths, bases, ref = [], [], [], []
    z = [0] * 6
    inserted = [[0, 0, 5, 0], [0, 0, 0, 5]]
    for name, rule, c, d, _, _ in COUNT_PAIRS:
        if rule == "base":                                           # G: c over both strands; the rest of the depth shows A on strand 1
            counts.append([[0, c - 7, 0, 0, 0, 9], [d - c, 7, 0, 0, 0, 0]])
            lengths.append([0, 0, 0])
            bases.append([[0] * 4] * 2)
        else:                                                        # the whole depth shows A; n sits in the column of length 2
            counts.append([[d, 0, 0, 0, 0, 0], z])
            lengths.append([0, c, 0])
            bases.append(inserted)
        ref.append(1)
    counts += [[[0, 0, 0, 0, NUM * K - 6, 0], [K - 1, 0, 0, 0, 7, 3]],                          # the deletion wins by one
               [[2 ** 30, 0, 0, 0, 0, 0], [2 ** 30 - 2, 0, 0, 0, 0, 5]],                        # d = 2^31 - 2
               [[2 ** 30, 0, 0, 0, 0, 5], [2 ** 30 - 1, 0, 0, 0, 0, 0]],                        # d = 2^31 - 1
               [[0, SPLIT[0], 0, 0, 0, 0], [0, SPLIT[1], 0, 0, 0, 0]]]                          # the strand sum is 2^31 - 1
    lengths += [[0, 0, 0], [0, 0, TOP], [0, 0, TOP], [1, 0, 0]]
    bases += [[[0] * 4] * 2, inserted, inserted, inserted]
    ref += [1, 2, 2, 1]
    pile = P.Pile(np.array(counts, dtype=np.int64), np.array(lengths, dtype=np.int64), np.array(bases, dtype=np.int64), None, 0)
    return Rows(pile, np.array(ref, dtype=np.int64))


# ---- every kind of record -------------------------------------------------------------------------------------------------------

VARIANT_R = T + 3
VARIANT_MAX_INS = 3
VARIANT_RULES = dict(min_depth=3, num=1, den=2)
# forced rows: position -> what it shows ("del", "keep", "sub", "ins": an insertion after a kept base, "sub+ins", "del+ins")
VARIANT_FORCED = {0: "del", 1: "del", 2: "keep",                                                # a deletion run at position 0
                  9: "keep", 10: "del", 11: "del", 12: "keep", 13: "del", 14: "keep",           # two runs one kept position apart
                  19: "keep", 20: "del", 21: "sub", 22: "del", 23: "ins", 24: "del", 25: "keep",            # runs beside other records
                  30: "keep", 31: "sub+ins", 32: "keep", 35: "keep", 36: "del+ins", 37: "keep",
                  VARIANT_R - 3: "keep", VARIANT_R - 2: "del", VARIANT_R - 1: "del"}            # a deletion run that ends at R - 1


def _show(pile, ref, p, what, rng):
    pile.counts[p], pile.ins_lengths[p], pile.ins_bases[p] = 0, 0, 0
    r = int(ref[p])
    if "del" in what:
        pile.counts[p, :, P.DEL] = (5, 4)
    elif "sub" in what:
        pile.counts[p, :, (r - 1 + int(rng.integers(1, 4))) % 4] = (3, 6)
    else:
        pile.counts[p, :, r - 1] = (4, 5)
    if "ins" in what:
        n = int(rng.integers(1, VARIANT_MAX_INS + 2))                # a length in 1..max_ins + 1
        pile.ins_lengths[p, n - 1] = 8
        for k in range(min(n, VARIANT_MAX_INS)):
            pile.ins_bases[p, k, int(rng.integers(0, 4))] = 8


@functools.lru_cache(maxsize=None)
def variants():
    """Rows over R = T + 3: random small counts, then a skewed draw of what every position shows, then the forced rows"""
    rng = np.random.default_rng(107)
    R = VARIANT_R
    pile, ref = random_pile(rng, R, VARIANT_MAX_INS, top=2), rng.integers(1, 5, size=R)
    kinds = ("keep", "sub", "del", "ins", "sub+ins", "noise")
    for p in range(R):
        what = VARIANT_FORCED.get(p) or kinds[int(rng.choice(len(kinds), p=[0.3, 0.15, 0.2, 0.1, 0.1, 0.15]))]
        if what != "noise":
            _show(pile, ref, p, what, rng)
    return Rows(pile, ref)


@functools.lru_cache(maxsize=None)
def variant_calls():
    rows = variants()
    return P.call_consensus_ref(rows.pile, rows.ref, **VARIANT_RULES)
