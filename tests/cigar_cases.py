"""The cases of the CIGAR encoder and decoder (csrc/wn_cigar.hip), built once and shared by
tests/test_cigar_ref.py and tests/test_gpu_cigar.py.  An op row is given in WALK orientation (front to back on the forward strand)
and stored in read orientation, reversed on strand 1; its labels are made to fit it: the reference label under op 1, another one
under op 2, so that the = / X split of a row is true against the labels and decode(encode(row)) can be compared column by column."""
import functools
import itertools
from collections import namedtuple

import numpy as np

from tests import cigar_ref as C

Batch = namedtuple("Batch", "names ops ops_len lo ref_len strand query query_len reference keep")
Runs = namedtuple("Runs", "names cigar n_cigar pos strand query query_len reference max_ops")

R = 4096
TILE = 256
EXAMPLE = [4, 4, 3, 1, 1, 2, 4, 1, 3, 3, 1, 4, 3]     # the worked example of include/wavenet_amd.h, READ orientation; lo 10


def reference_labels(n=R, seed=99):
    return np.random.default_rng(seed).integers(1, 5, size=n).astype(np.int32)


def fit_query(walk, lo, reference, rng):
    """the query labels in FORWARD orientation that fit a walk-orientation op row at window start lo"""
    out, i = [], 0
    for op in walk:
        r = int(reference[lo + i]) if op != 4 else 0
        if op != 3:
            out.append(r if op == 1 else r % 4 + 1 if op == 2 else int(rng.integers(1, 5)))
        i += op != 4
    return out


def read_orientation(seq, strand, complement):
    seq = list(seq)
    if strand != 1:
        return seq
    return [5 - v for v in seq[::-1]] if complement else seq[::-1]


def assemble(rows, reference, seed, lo_step=3, width=None, keep=None):
    """rows: [(name, walk-orientation ops, strand)] -> Batch; lo = 5 + lo_step * b"""
    rng = np.random.default_rng(seed)
    B = len(rows)
    W = max([len(r[1]) for r in rows] + [1]) if width is None else width
    lo = (5 + lo_step * np.arange(B)).astype(np.int32)
    queries = [fit_query(walk, int(lo[b]), reference, rng) for b, (_, walk, _) in enumerate(rows)]
    Mq = max([len(q) for q in queries] + [1])
    ops, query = np.zeros((B, W), dtype=np.uint8), np.zeros((B, Mq), dtype=np.int32)
    ops_len, ref_len, query_len, strand = (np.zeros(B, dtype=np.int32) for _ in range(4))
    for b, (_, walk, s) in enumerate(rows):
        ops[b, :len(walk)] = read_orientation(walk, s, False)
        query[b, :len(queries[b])] = read_orientation(queries[b], s, True)
        ops_len[b], ref_len[b], query_len[b], strand[b] = len(walk), sum(v != 4 for v in walk), len(queries[b]), s
    assert int((lo + ref_len).max()) <= len(reference)
    return Batch([r[0] for r in rows], ops, ops_len, lo, ref_len, strand, query, query_len, reference,
                 np.ones(B, dtype=bool) if keep is None else np.asarray(keep, dtype=bool))


def random_walk(rng, n, gaps=(3, 4, 4)):
    """n columns, first and last aligned (n >= 1)"""
    row = [int(v) for v in rng.choice([1] * 7 + [2, 2] + list(gaps), size=n)]
    if n:
        row[0], row[-1] = 1, int(rng.integers(1, 3))
    return row


def own_runs(n):
    """n columns of which each is a run of its own, with = / X and with M: the cycle = D X I, aligned at both ends"""
    return ([1, 3, 2, 4] * (n // 4 + 1))[:n - 1] + [1]


def shapes():
    """[(name, walk-orientation ops)]: the lengths, the run placements and the degenerate rows"""
    rng = np.random.default_rng(2024)
    rows = [("len%d" % n, random_walk(rng, n)) for n in (0, 1, 255, 256, 257, 511, 512, 513, 1100)]
    rows.append(("heads_63_64_255_256", [1] * 63 + [2] + [3] + [1] * 190 + [4] + [2] + [1] * 20))
    rows.append(("match_run_700", [2] * 30 + [1] * 700 + [4, 1, 1]))
    rows.append(("deletion_250_262", [1] * 250 + [3] * 13 + [1] * 40))
    rows.append(("own_runs_600", own_runs(600)))
    rows.append(("one_aligned", [4, 4, 3, 1, 3, 4]))
    rows.append(("all_insertion", [4] * 20))                          # ref_lengths 0: skipped
    rows.append(("no_aligned", [3, 4, 4, 3, 3]))                      # used 0: end columns only
    rows.append(("end_mixes", [3, 4, 3, 3, 4, 1, 2, 1, 4, 3, 1, 4, 3, 4, 4, 3]))
    rows.append(("clips_over_tiles", [4] * 300 + [3] * 5 + random_walk(rng, 40) + [3] * 2 + [4] * 270))
    rows.append(("example", list(EXAMPLE)))
    return rows


@functools.lru_cache(maxsize=None)
def encode_batch():
    """every shape on both strands; `keep` drops two reads"""
    rows = [(name + "/%d" % s, walk if s == 0 or name != "example" else walk[::-1], s) for name, walk in shapes() for s in (0, 1)]
    # the example is given in READ orientation: on strand 1 its walk is the row reversed, and assemble() reverses it back
    keep = np.ones(len(rows), dtype=bool)
    keep[[4, 9]] = False
    return assemble(rows, reference_labels(), 7, keep=keep)


@functools.lru_cache(maxsize=None)
def overflow_batch():
    """600 runs exactly, and the same row behind a front clip: 601 -> (Batch, max_cigar)"""
    rows = [("exact/0", own_runs(600), 0), ("over/0", [4] + own_runs(600), 0), ("exact/1", own_runs(600), 1), ("over/1", own_runs(600) + [4], 1)]
    return assemble(rows, reference_labels(), 11), 600


@functools.lru_cache(maxsize=None)
def limit_read():
    """one read at the limits: 8192 query labels in 65535 + 8192 columns, most of them one deletion run"""
    rng = np.random.default_rng(5)
    body = [int(v) for v in rng.choice([1] * 8 + [2, 4], size=8192)]
    body[0] = body[-1] = 1
    walk = body[:4000] + [3] * 65535 + body[4000:]
    return assemble([("limit/0", walk, 0), ("limit/1", walk, 1)], reference_labels(80000, 3), 13, lo_step=100)


def bad_window(batch, b):
    """a copy of a Batch whose read b has its window end past the reference"""
    lo = batch.lo.copy()
    lo[b] = len(batch.reference) - int(batch.ref_len[b]) + 1
    return batch._replace(lo=lo)


def words(runs):
    """[(len, code)] as the int32 bit patterns of the 32-bit words"""
    return [v - (1 << 32) if v >= 1 << 31 else v for v in C.pack(runs)]


def runs_batch(rows, reference, max_ops, width=None):
    """rows: [(name, [(len, code)] or raw words, pos, strand, query in READ orientation, query_len or None, n_cigar or None)] -> Runs"""
    B = len(rows)
    cig = [words(r[1]) if r[1] and isinstance(r[1][0], tuple) else list(r[1]) for r in rows]
    W = max([len(c) for c in cig] + [1]) if width is None else width
    Mq = max([len(r[4]) for r in rows] + [1])
    cigar, query = np.zeros((B, W), dtype=np.int32), np.zeros((B, Mq), dtype=np.int32)
    n_cigar, pos, strand, query_len = (np.zeros(B, dtype=np.int32) for _ in range(4))
    for b, (_, _, p, s, q, n_q, n_c) in enumerate(rows):
        cigar[b, :len(cig[b])], query[b, :len(q)] = cig[b], q
        n_cigar[b], pos[b], strand[b], query_len[b] = len(cig[b]) if n_c is None else n_c, p, s, len(q) if n_q is None else n_q
    return Runs([r[0] for r in rows], cigar, n_cigar, pos, strand, query, query_len, reference, max_ops)


def labels_under(runs, pos, strand, reference, rng, wrong=()):
    """the query in READ orientation that fits runs at pos: the reference label under = and M, another under X; `wrong` lists
    forward query indices whose label is changed afterwards"""
    fwd, i = [], pos
    for n, c in runs:
        for _ in range(n):
            if c in (C.M, C.EQ, C.X):
                r = int(reference[i])
                fwd.append(r % 4 + 1 if c == C.X else r)
            elif c in (C.I, C.S):
                fwd.append(int(rng.integers(1, 5)))
            i += c in (C.M, C.EQ, C.X, C.D)
    for j in wrong:
        fwd[j] = fwd[j] % 4 + 1
    return read_orientation(fwd, strand, True)


@functools.lru_cache(maxsize=None)
def decode_batch():
    """hand-made run tables: the codes that vanish, the bad kinds, the skipped kinds, sums that would wrap 32 bits"""
    ref, rng = reference_labels(), np.random.default_rng(31)
    P = C.parse
    rows = []

    def add(name, runs, pos=20, strand=0, wrong=(), n_query=None, n_cigar=None, query=None, labels_of=None):
        q = labels_under(labels_of or runs, pos, strand, ref, rng, wrong) if query is None else query
        rows.append((name, runs, pos, strand, q, n_query, n_cigar))

    for s in (0, 1):
        add("plain/%d" % s, P("5S10=2X3I4=2D6=1S"), strand=s)
        add("vanishing/%d" % s, P("5H3S0M4=1P2I0D3X2D1=0I2S4H"), strand=s)
        add("m_runs/%d" % s, P("6M1I7M2D3M"), strand=s, wrong=(2, 9))
        add("eq_over_mismatch/%d" % s, P("8=2I5="), strand=s, wrong=(3,))          # strict: bad
        add("x_over_match/%d" % s, P("4=1X4="), strand=s, labels_of=P("9="))       # strict: bad
        add("other_label/%d" % s, P("3=1X2="), strand=s, query=[0, 7, 1, 2, 3, 4])
    add("n_run", P("3=2N3="))
    add("code_9", [(3, C.EQ), (2, 9), (3, C.EQ)], query=[1] * 8)
    add("code_15_len_0", [(3, C.EQ), (0, 15), (3, C.EQ)], query=[1] * 6)
    add("strand_2", P("6="), strand=2, query=[1] * 6)
    add("strand_-1", P("6="), strand=-1, query=[1] * 6)
    add("n_cigar_0", P("6="), n_cigar=0, query=[1] * 6)
    add("n_cigar_-1", P("6="), n_cigar=-1, query=[1] * 6)
    add("n_cigar_over", P("6="), n_cigar=10 ** 6, query=[1] * 6)
    add("pos_-1", P("6="), pos=-1, query=[1] * 6)
    add("pos_last", P("6="), pos=R - 6)
    add("pos_past", P("6="), pos=R - 5, query=[1] * 6)
    add("pos_far", P("6="), pos=2 ** 31 - 3, query=[1] * 6)
    add("no_reference", P("3S4I"), query=[1] * 7)
    add("only_deletion", P("4D"), query=[])                             # consumes a reference label and no query label: valid
    add("query_short", P("6="), n_query=5)
    add("query_long", P("6="), n_query=7)
    add("query_len_-1", P("6="), n_query=-1)
    add("query_len_over", P("6="), n_query=10 ** 6)
    add("columns_at_max", P("30=20D14="))                               # 64 columns = max_ops
    add("columns_over", P("30=21D14="))
    top = C.MAX_LEN
    add("wrap_columns", [(top, C.EQ)] * 16 + [(16, C.EQ)] + P("6="), query=[1] * 6)     # 2^32 + 6 columns, reference and query labels
    add("wrap_query", [(top, C.S)] * 16 + [(16, C.S)] + P("6="), query=[1] * 6)
    add("wrap_reference", [(top, C.D)] * 16 + [(16, C.D)] + P("6="), query=[1] * 6)
    add("wrap_to_negative", [(top, C.EQ)] * 8 + [(8, C.EQ)] + P("6="), query=[1] * 6)   # 2^31 + 6
    return runs_batch(rows, ref, 64)


@functools.lru_cache(maxsize=None)
def run_edge_batch():
    """rows of 255, 256 and 257 runs (every column a run of its own), and one of 1100, on both strands, as run tables"""
    ref = reference_labels()
    batch = assemble([("runs%d/%d" % (n, s), own_runs(n), s) for n in (255, 256, 257, 1100) for s in (0, 1)], ref, 17)
    enc = C.encode_ref(batch.ops, batch.ops_len, batch.lo, batch.ref_len, batch.strand, batch.query_len, batch.query.shape[1], len(ref))
    assert enc.n_cigar.tolist() == [255, 255, 256, 256, 257, 257, 1100, 1100]
    return batch, Runs(batch.names, enc.cigar.view(np.int32), enc.n_cigar, enc.fields[:, 0].copy(), batch.strand, batch.query, batch.query_len, ref,
                       batch.ops.shape[1])


def random_batch(seed, B=48, n_max=700):
    """random rows with long end mixes on both strands, for the round trips"""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(B):
        ends = [[int(v) for v in rng.choice([3, 4], size=int(rng.integers(0, 6)))] for _ in range(2)]
        rows.append(("random%d" % b, ends[0] + random_walk(rng, int(rng.integers(1, n_max))) + ends[1], b & 1))
    return assemble(rows, reference_labels(), seed + 1, lo_step=40)


def all_rows(max_len=6):
    """every op row of 1..max_len columns over the ops 1..4, in walk orientation"""
    for n in range(1, max_len + 1):
        for row in itertools.product((1, 2, 3, 4), repeat=n):
            yield list(row)


def walk_of(batch, b):
    """the walk-orientation ops of read b"""
    row = [int(v) for v in batch.ops[b, :batch.ops_len[b]]]
    return row[::-1] if batch.strand[b] == 1 else row


def round_trip_row(walk, enc_row_fields):
    """[4] * clip_front + walk[first..last] + [4] * clip_back: what decode(encode(row)) is in walk orientation"""
    aligned = [w for w, v in enumerate(walk) if v <= 2]
    return [4] * int(enc_row_fields[2]) + walk[aligned[0]:aligned[-1] + 1] + [4] * int(enc_row_fields[3])


def cigar_rows(enc, strand, eqx=True, to=None):
    """the Rows of cigar_ref.encode_ref as the CigarRows of the package: host tensors, or through `to` (tests.gpu_util.dev)"""
    import torch
    import wavenet_speech_amd as W
    to = to or (lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    f = enc.fields.astype(np.int32)
    return W.CigarRows(to(enc.cigar.view(np.int32)), to(enc.n_cigar.astype(np.int32)), to(f[:, 0]), to(f[:, 1]), to(f[:, 2]), to(f[:, 3]), to(f[:, 4]),
                       to(enc.used), eqx, to(np.asarray(strand, dtype=np.int32)))


# a reference for the MD strings of the SAM tag specification: A at 10, AC at 16, T at 18
MD_LETTERS = "C" * 10 + "A" + "C" * 5 + "ACT" + "C" * 20

# the SAM specification's example (section 1.1): the reference without its pads, and the reads the tests use
SPEC_REFERENCE = "AGCATGTTAGATAAGATAGCTGTGCTAGTAGGCAGTCAGCGCCAT"
SPEC_READS = (("r001", 7, "8M2I4M1D3M", "TTAGATAAAGGATACTG"), ("r002", 9, "3S6M1P1I4M", "AAAAGATAAGGATA"), ("r003", 9, "5S6M", "GCCTAAGCTAA"),
              ("r003h", 9, "5H6M", "AGCTAA"), ("r003s", 29, "6H5M", "TAGGC"))
