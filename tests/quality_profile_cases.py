"""The inputs of tests/test_gpu_profile.py, built on the CPU from fixed seeds (numpy only), with the loop reference of each
(tests/quality_profile_ref.py) computed once and shared.  Op strings are random consistent walks: the ops are drawn first and
the two label rows are written to fit them, so nothing here goes through the aligner."""
import functools

import numpy as np

from tests import quality_profile_ref as PR

# the edges of the scan: one wave (64), one tile (256), and their neighbours; 1200 is five tiles, the last one partial
OPS_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 1200)


def random_ops(rng, n, weights=(0.7, 0.1, 0.1, 0.1)):
    """n op codes 1..4"""
    return rng.choice(np.arange(1, 5), size=n, p=np.asarray(weights) / np.sum(weights)).astype(np.uint8)


def rows_for(rng, ops, classes, lowest=0):
    """(ref, query): label lists in [lowest, classes) that the ops are a valid alignment of"""
    ref, query = [], []
    for op in ops:
        x = int(rng.integers(lowest, classes))
        if op == 1:
            ref.append(x); query.append(x)
        elif op == 2:
            y = int(rng.integers(lowest, classes - 1))
            ref.append(x); query.append(y if y < x else y + 1)
        elif op == 3:
            ref.append(x)
        else:
            query.append(x)
    return ref, query


class Batch(object):
    """ops [B, W] uint8 zero-padded, ref [B, N] / query [B, M] int32 padded with `fill`, their lengths (int32), qual [B, M] uint8 in
    0..93, dwell [B, M] int32 in 0..50 (so rows above 32 occur)"""

    def __init__(self, seed, op_rows, classes, fill=0, lowest=0, extra_width=0):
        rng = np.random.default_rng(seed)
        self.classes = classes
        pairs = [rows_for(rng, ops, classes, lowest) for ops in op_rows]
        B = len(op_rows)
        N = max([len(r) for r, _ in pairs] + [1]) + extra_width
        M = max([len(q) for _, q in pairs] + [1]) + extra_width
        W = max([len(o) for o in op_rows] + [1]) + extra_width
        self.ops = np.zeros((B, W), dtype=np.uint8)
        self.ref = np.full((B, N), fill, dtype=np.int32)
        self.query = np.full((B, M), fill, dtype=np.int32)
        for b, (ops, (r, q)) in enumerate(zip(op_rows, pairs)):
            self.ops[b, :len(ops)] = ops
            self.ref[b, :len(r)] = r
            self.query[b, :len(q)] = q
        self.ops_len = np.array([len(o) for o in op_rows], dtype=np.int32)
        self.ref_len = np.array([len(r) for r, _ in pairs], dtype=np.int32)
        self.query_len = np.array([len(q) for _, q in pairs], dtype=np.int32)
        self.qual = rng.integers(0, 94, size=(B, M)).astype(np.uint8)
        self.dwell = rng.integers(0, 51, size=(B, M)).astype(np.int32)

    def copy(self):
        other = object.__new__(Batch)
        other.__dict__ = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()}
        return other

    def take(self, rows):
        other = self.copy()
        for k, v in other.__dict__.items():
            if isinstance(v, np.ndarray):
                other.__dict__[k] = v[rows].copy()
        return other

    @property
    def max_ops(self):
        return min(self.ops.shape[1], self.ref.shape[1] + self.query.shape[1])

    def reference(self, count_ends, qual=True, dwell=True, into=None):
        return PR.profile(self.ops, self.ops_len, self.ref, self.ref_len, self.query, self.query_len,
                          self.qual if qual else None, self.dwell if dwell else None, self.classes, count_ends, into=into)


def _edges(seed, classes, lengths):
    rng = np.random.default_rng(seed)
    return Batch(seed + 1, [random_ops(rng, n) for n in lengths], classes)


def _special(seed, classes):
    """the alignments a walk rarely draws"""
    rng = np.random.default_rng(seed)
    u8 = lambda v: np.asarray(v, dtype=np.uint8)  # noqa: E731
    rows = [
        u8([3] * 40 + [4] * 30),                                     # no match or mismatch column at all: every column an end column
        u8([3] * 70 + [4] * 90 + [1] + list(random_ops(rng, 300)) + [2] + [4] * 5 + [3] * 7),   # a head of op 3s, then op 4s
        u8([]),                                                      # an empty read against an empty reference
        u8([4] * 300),                                               # a read against an empty reference
        u8([3] * 257),                                               # a reference against an empty read
        u8([1]),
        u8([2] + [3] * 255 + [2]),                                   # lo and hi in different tiles, a tile boundary between them
        u8([4] * 256 + [1] + [4] * 256),                             # the only aligned column is the first of the second tile
    ]
    return Batch(seed + 1, rows, classes)


CASES = {
    "edges_c5": lambda: _edges(11, 5, OPS_LENGTHS + (300,)),                       # 12 reads: one to five tiles share a launch
    "edges_c64": lambda: _edges(12, 64, (1200, 1, 257, 64, 513, 0, 255)),
    "edges_c5_b4": lambda: _edges(13, 5, (511, 63, 256, 65)),
    "special_c5": lambda: _special(14, 5),
    "special_c64": lambda: _special(15, 64),
    "one_class": lambda: Batch(16, [random_ops(np.random.default_rng(16), 300, (0.8, 0.0, 0.1, 0.1)), np.zeros(0, np.uint8),
                                    np.ones(64, np.uint8), np.full(3, 4, np.uint8)], 1),   # classes = 1: no mismatch can exist
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, count_ends, qual=True, dwell=True):
    """the reference of a case; shared, so do not write into it"""
    return case(name).reference(count_ends, qual, dwell)


# ---- bad reads: a batch of good reads, and the same batch with one bad copy of each kind between them
BAD_KINDS = ("op code 5", "a 0 inside ops_len", "consumed counts off by one", "op 1 over unequal labels", "a label equal to classes",
             "qual of 94", "ops_len = max_ops + 1", "a length of -1")


@functools.lru_cache(maxsize=None)
def bad_batches():
    """(good, mixed, bad_rows): `mixed` holds the reads of `good` in order with 8 bad reads between them; bad_rows are their
    indices in `mixed`.  Both batches have the same widths, so the same max_ops."""
    rng = np.random.default_rng(21)
    lengths = (65, 257, 300, 40, 513, 128)
    good = Batch(22, [random_ops(rng, n) for n in lengths], 5, extra_width=3)
    order = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 0, 3]               # a bad copy after each good read, and two more at the end
    mixed = good.take(order)
    bad_rows = [1, 3, 5, 7, 9, 11, 12, 13]
    b = bad_rows[0]                                                  # op code 5
    mixed.ops[b, 30] = 5
    b = bad_rows[1]                                                  # a 0 inside ops_len, in the second tile
    mixed.ops[b, 256] = 0
    b = bad_rows[2]                                                  # the ops consume one more reference label than ref_len
    mixed.ref_len[b] -= 1
    b = bad_rows[3]                                                  # an op 1 over unequal labels
    c = int(np.nonzero(mixed.ops[b, :mixed.ops_len[b]] == 1)[0][3])
    j = int((mixed.ops[b, :c] != 3).sum())
    mixed.query[b, j] = (mixed.query[b, j] + 1) % 5
    b = bad_rows[4]                                                  # a label equal to classes, under a deletion in the last tile
    c = int(np.nonzero(mixed.ops[b, :mixed.ops_len[b]] == 3)[0][-1])
    mixed.ref[b, int((mixed.ops[b, :c] != 4).sum())] = 5
    b = bad_rows[5]                                                  # qual of 94
    mixed.qual[b, 17] = 94
    assert mixed.query_len[b] > 17
    b = bad_rows[6]                                                  # ops_len = max_ops + 1
    mixed.ops_len[b] = mixed.max_ops + 1
    b = bad_rows[7]                                                  # a length of -1
    mixed.query_len[b] = -1
    assert good.max_ops == mixed.max_ops
    return good, mixed, bad_rows


# ---- end to end: true labels and a mutated copy, for the project's own aligner
def mutated_pairs(seed=31, B=6, lo=150, hi=420, rate=0.06):
    """ragged_reads-style truth (labels 1..4, zero-padded) and a copy with substitutions, insertions and deletions, each at
    `rate` of the positions, plus a few extra labels at the copy's head and tail"""
    rng = np.random.default_rng(seed)
    truth, calls = [], []
    for _ in range(B):
        t = rng.integers(1, 5, size=int(rng.integers(lo, hi))).tolist()
        q = rng.integers(1, 5, size=int(rng.integers(0, 6))).tolist()
        for v in t:
            u = rng.random()
            if u < rate:
                q.append(1 + (v + int(rng.integers(0, 3))) % 4)       # a substitution
            elif u < 2 * rate:
                continue                                             # a deletion
            else:
                q.append(v)
            if rng.random() < rate:
                q.append(int(rng.integers(1, 5)))                    # an insertion
        q += rng.integers(1, 5, size=int(rng.integers(0, 6))).tolist()
        truth.append(t); calls.append(q)

    def pad(rows):
        out = np.zeros((len(rows), max(len(r) for r in rows)), dtype=np.int32)
        for b, r in enumerate(rows):
            out[b, :len(r)] = r
        return out, np.array([len(r) for r in rows], dtype=np.int32)
    return pad(truth), pad(calls)
