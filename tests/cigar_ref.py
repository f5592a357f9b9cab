"""CPU reference of the CIGAR encoder and decoder and of the MD tag (csrc/wn_cigar.hip, wavenet_speech_amd/sam.py; DESIGN.md section
7ac), as plain loops over Python integers, written from the definitions in include/wavenet_amd.h and not from the kernels: a row is
turned into walk orientation first (reversed on strand 1), so that everything below reads front to back on the forward strand.

Ops: 1 match, 2 mismatch, 3 reference label against a gap, 4 query label against a gap.  Labels 1..4 = A, G, C, T, the complement
of v is 5 - v.  A run is len << 4 | code with BAM's codes, CODES[code] its letter.  tests/test_cigar_ref.py holds this file to the
worked example, to the SAM specification's own reads and to an exhaustive enumeration of short rows."""
from collections import namedtuple

import numpy as np

from tests import pileup_ref as P

CODES = "MIDNSHP=X"
M, I, D, N, S, H, PAD, EQ, X = range(9)
MAX_LEN = (1 << 28) - 1

Encoded = namedtuple("Encoded", "used runs pos ref_span clip_front clip_back nm")     # runs: [(len, code)], all of them
Rows = namedtuple("Rows", "cigar n_cigar fields used bad")
Decoded = namedtuple("Decoded", "used ops ref_len stats")                               # ops: the row in READ orientation
OpRows = namedtuple("OpRows", "ops ops_len ref_lengths stats used bad")


def pack(runs):
    return [(n << 4) | c for n, c in runs]


def unpack(words):
    return [((int(v) & 0xFFFFFFFF) >> 4, int(v) & 15) for v in words]      # a word may come as its int32 bit pattern


def text(runs):
    return "".join("%d%s" % (n, CODES[c]) for n, c in runs)


def parse(string):
    """'8M2I4M' -> [(8, 0), (2, 1), (4, 0)]"""
    runs, n = [], ""
    for ch in string:
        if ch.isdigit():
            n += ch
        else:
            runs.append((int(n), CODES.index(ch)))
            n = ""
    return runs


def encode_row(ops, ops_len, max_ops, lo, n_ref, strand, n_query, max_query, R, eqx=True, keep=True):
    """one read -> Encoded; used is 1, 0 or -1 here (the -2 of a row that does not fit is encode_ref's: it needs max_cigar)"""
    state = P.read_state(ops, ops_len, max_ops, lo, n_ref, strand, n_query, max_query, R, None, keep)
    walk = [int(v) for v in ops[:ops_len]][::-1 if strand == 1 else 1] if state == 1 else []
    aligned = [w for w, v in enumerate(walk) if v <= 2]
    if state != 1 or not aligned:
        return Encoded(state if state != 1 else 0, [], -1, 0, 0, 0, 0)
    first, last = aligned[0], aligned[-1]
    i = lambda w: sum(v != 4 for v in walk[:w])                      # noqa: E731  the reference labels consumed before w
    j = lambda w: sum(v != 3 for v in walk[:w])                      # noqa: E731  the query labels consumed before w
    clip_front, clip_back = j(first), n_query - j(last) - 1
    code = {1: EQ if eqx else M, 2: X if eqx else M, 3: D, 4: I}
    runs = []
    for w in range(first, last + 1):
        c = code[walk[w]]
        if runs and runs[-1][1] == c:
            runs[-1] = (runs[-1][0] + 1, c)
        else:
            runs.append((1, c))
    runs = ([(clip_front, S)] if clip_front > 0 else []) + runs + ([(clip_back, S)] if clip_back > 0 else [])
    nm = sum(walk[w] >= 2 for w in range(first, last + 1))
    return Encoded(1, runs, lo + i(first), i(last) - i(first) + 1, clip_front, clip_back, nm)


def encode_ref(ops, ops_len, lo, ref_lengths, strand, query_lengths, max_query, R, eqx=True, max_cigar=None, keep=None):
    """ops [B][max_ops] -> Rows: cigar [B][max_cigar] uint32, n_cigar [B], fields [B][5], used [B] int8, bad: the count"""
    B = len(ops_len)
    max_ops = len(ops[0]) if B else 0
    if max_cigar is None:
        max_cigar = min(max_ops, 2 * max_query + 1) + 2
    cigar, n_cigar = np.zeros((B, max_cigar), dtype=np.uint32), np.zeros(B, dtype=np.int32)
    fields, used, bad = np.zeros((B, 5), dtype=np.int32), np.zeros(B, dtype=np.int8), 0
    for b in range(B):
        e = encode_row(ops[b], int(ops_len[b]), max_ops, int(lo[b]), int(ref_lengths[b]), int(strand[b]), int(query_lengths[b]), max_query, R,
                       eqx, True if keep is None else bool(keep[b]))
        state = -2 if len(e.runs) > max_cigar else e.used
        if state == 1:
            cigar[b, :len(e.runs)] = pack(e.runs)
        n_cigar[b], used[b] = len(e.runs), state
        fields[b] = (e.pos, e.ref_span, e.clip_front, e.clip_back, e.nm)
        bad += state < 0
    return Rows(cigar, n_cigar, fields, used, bad)


def forward_label(v, strand):
    v = int(v)
    return 5 - v if strand == 1 and 1 <= v <= 4 else v


def decode_row(words, n_cigar, pos, strand, reference, query, n_query, max_cigar, max_query, max_ops, strict=False):
    """one read's runs (uint32 words) -> Decoded"""
    skipped, bad = Decoded(0, [], 0, [0, 0, 0, 0]), Decoded(-1, [], 0, [-1, -1, -1, -1])
    if strand < 0 or n_cigar == 0:
        return skipped
    if strand > 1 or not 0 <= n_cigar <= max_cigar or pos < 0 or not 0 <= n_query <= max_query:
        return bad
    runs = unpack(words[:n_cigar])
    if any(c > X or c == N for _, c in runs):
        return bad
    n_cols = sum(n for n, c in runs if c not in (H, PAD))
    n_ref = sum(n for n, c in runs if c in (M, EQ, X, D))
    if n_cols > max_ops or n_ref < 1 or pos + n_ref > len(reference) or sum(n for n, c in runs if c in (M, EQ, X, I, S)) != n_query:
        return bad
    walk, i, j = [], 0, 0
    for n, c in runs:
        for _ in range(n):
            if c in (M, EQ, X):
                equal = int(reference[pos + i]) == forward_label(query[n_query - 1 - j] if strand == 1 else query[j], strand)
                if strict and ((c == EQ and not equal) or (c == X and equal)):
                    return bad
                walk.append(1 if equal else 2)
                i, j = i + 1, j + 1
            elif c in (I, S):
                walk.append(4)
                j += 1
            elif c == D:
                walk.append(3)
                i += 1
    stats = [walk.count(1), walk.count(2), walk.count(3) + walk.count(4), len(walk)]
    return Decoded(1, walk[::-1] if strand == 1 else walk, n_ref, stats)


def decode_ref(cigar, n_cigar, pos, strand, reference, query, query_lengths, max_ops, strict=False):
    """cigar [B][max_cigar], query [B][M] -> OpRows: ops [B][max_ops] uint8, ops_len, ref_lengths [B], stats [B][4], used, bad"""
    B = len(n_cigar)
    max_cigar, max_query = len(cigar[0]), len(query[0])
    ops, ops_len, ref_len = np.zeros((B, max_ops), dtype=np.uint8), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    stats, used, bad = np.zeros((B, 4), dtype=np.int32), np.zeros(B, dtype=np.int8), 0
    for b in range(B):
        d = decode_row(cigar[b], int(n_cigar[b]), int(pos[b]), int(strand[b]), reference, query[b], int(query_lengths[b]), max_cigar,
                       max_query, max_ops, strict)
        ops[b, :len(d.ops)] = d.ops
        ops_len[b], ref_len[b], stats[b], used[b] = len(d.ops), d.ref_len, d.stats, d.used
        bad += d.used < 0
    return OpRows(ops, ops_len, ref_len, stats, used, bad)


def md_ref(runs, pos, letters):
    """the MD:Z text of =/X runs at `pos` of a reference given as a string"""
    out, u, at = "", 0, pos
    for n, c in runs:
        if c == EQ:
            u, at = u + n, at + n
        elif c == X:
            for _ in range(n):
                out, u, at = out + "%d%s" % (u, letters[at]), 0, at + 1
        elif c == D:
            out, u, at = out + "%d^%s" % (u, letters[at:at + n]), 0, at + n
        elif c == M:
            raise ValueError("MD needs = / X runs")
    return out + "%d" % u
