"""CPU reference of global pairwise alignment with affine gaps (Gotoh), numpy int64, for csrc/wn_pairalign.hip.

`a` is the reference (rows i = 1..N), `b` the query (columns j = 1..M); a gap of length n costs go + (n - 1) ge.

    E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge)       a column of b against a gap; opening wins a tie (bit 0, extend 1)
    F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)       a row of a against a gap; the same tie rule
    H[i][j] = diag = H[i-1][j-1] + (match | mismatch), then E, then F: a later one replaces an earlier one only if strictly greater
    borders   E[i][0] = F[0][j] = -inf, H[0][0] = 0, H[i][0] and H[0][j] are 0 with free end gaps, else -(go + ge (k - 1))
    end cell  (N, M); with free end gaps start from (N, M), scan the last row j = M..0, then the last column i = N..0, and
              replace only on strictly greater
    trace     the H / E / F state machine back from the end cell until i == 0 or j == 0; the unconsumed head and tail of
              either sequence are end gaps: they appear in the ops and count in `gaps` and `length`

The fill is vectorised over anti-diagonals (cells with i + j = d depend on the diagonals d - 1 and d - 2 only); the trace is a
plain loop.  Op codes: 1 match, 2 mismatch, 3 reference label against a gap, 4 query label against a gap.
tests/test_pairwise_align_ref.py holds this file to exhaustive enumeration, textbook Levenshtein and recorded EMBOSS needle
results."""
from collections import namedtuple

import numpy as np

NEG = -(1 << 40)
OP_MATCH, OP_MISMATCH, OP_REF_GAP, OP_QUERY_GAP = 1, 2, 3, 4
EMBOSS = (10, -8, 20, 1)            # needle's EDNAFULL 5 / -4, gap open 10, gap extend 0.5, in half units
UNIT = (0, -1, 1, 1)                # -score is the Levenshtein distance (with end gaps penalised)

Result = namedtuple("Result", "score matches mismatches gaps length ops")


def border(k, go, ge, free):
    return 0 if (free or k == 0) else -(go + ge * (k - 1))


def fill(a, b, match, mismatch, go, ge, free):
    """H [N+1][M+1] int64 and the backpointers [N+1][M+1] uint8: bits 0-1 H's choice (0 diag, 1 E, 2 F), bit 2 E, bit 3 F"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n, m = len(a), len(b)
    H = np.zeros((n + 1, m + 1), dtype=np.int64)
    E = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    F = np.full((n + 1, m + 1), NEG, dtype=np.int64)
    bp = np.zeros((n + 1, m + 1), dtype=np.uint8)
    if not free:
        H[1:, 0] = -(go + ge * np.arange(n, dtype=np.int64))
        H[0, 1:] = -(go + ge * np.arange(m, dtype=np.int64))
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        eo, ee = H[i, j - 1] - go, E[i, j - 1] - ge
        fo, fe = H[i - 1, j] - go, F[i - 1, j] - ge
        e, f = np.maximum(eo, ee), np.maximum(fo, fe)
        h = H[i - 1, j - 1] + np.where(a[i - 1] == b[j - 1], match, mismatch)
        k = np.zeros(len(i), dtype=np.uint8)
        pick = e > h
        h = np.where(pick, e, h)
        k[pick] = 1
        pick = f > h
        h = np.where(pick, f, h)
        k[pick] = 2
        H[i, j], E[i, j], F[i, j] = h, e, f
        bp[i, j] = k | ((ee > eo).astype(np.uint8) << 2) | ((fe > fo).astype(np.uint8) << 3)
    return H, bp


def end_cell(H, free):
    n, m = H.shape[0] - 1, H.shape[1] - 1
    best, bi, bj = H[n, m], n, m
    if free:
        for j in range(m, -1, -1):
            if H[n, j] > best:
                best, bi, bj = H[n, j], n, j
        for i in range(n, -1, -1):
            if H[i, m] > best:
                best, bi, bj = H[i, m], i, m
    return int(best), bi, bj


def align(a, b, match=EMBOSS[0], mismatch=EMBOSS[1], go=EMBOSS[2], ge=EMBOSS[3], free=True):
    """one pair -> Result(score, matches, mismatches, gaps, length, ops front to back as a uint8 array)"""
    n, m = len(a), len(b)
    H, bp = fill(a, b, match, mismatch, go, ge, free)
    score, i, j = end_cell(H, free)
    back = [OP_REF_GAP] * (n - i) + [OP_QUERY_GAP] * (m - j)         # the tail, back to front (at most one kind is present)
    st = 0
    while i > 0 and j > 0:
        v = int(bp[i, j])
        if st == 0:
            st = v & 3
            if st == 0:
                back.append(OP_MATCH if a[i - 1] == b[j - 1] else OP_MISMATCH)
                i, j = i - 1, j - 1
        elif st == 1:
            back.append(OP_QUERY_GAP)
            j -= 1
            if not v & 4:
                st = 0
        else:
            back.append(OP_REF_GAP)
            i -= 1
            if not v & 8:
                st = 0
    back += [OP_REF_GAP] * i + [OP_QUERY_GAP] * j
    ops = np.array(back[::-1], dtype=np.uint8)
    nm, nx = int((ops == OP_MATCH).sum()), int((ops == OP_MISMATCH).sum())
    return Result(score, nm, nx, len(ops) - nm - nx, len(ops), ops)


def score_only(a, b, match, mismatch, go, ge, free):
    H, _ = fill(a, b, match, mismatch, go, ge, free)
    return end_cell(H, free)[0]


def replay(a, b, ops):
    """the two sequences an op row spells (each must come out exactly once, in order): (ref labels, query labels)"""
    ra, rb, i, j = [], [], 0, 0
    for op in ops:
        if op in (OP_MATCH, OP_MISMATCH):
            assert (a[i] == b[j]) == (op == OP_MATCH), (i, j, op)
            ra.append(a[i]); rb.append(b[j])
            i, j = i + 1, j + 1
        elif op == OP_REF_GAP:
            ra.append(a[i])
            i += 1
        elif op == OP_QUERY_GAP:
            rb.append(b[j])
            j += 1
        else:
            raise AssertionError("op code %r" % (op,))
    return ra, rb


def rescore(ops, match, mismatch, go, ge, free):
    """the score of an op row under the cost model: gap runs of one kind cost go + (n - 1) ge; with free end gaps the runs that
    touch either end of the row cost nothing"""
    ops = [int(v) for v in ops]
    total, q, n = 0, 0, len(ops)
    while q < n:
        op = ops[q]
        if op == OP_MATCH:
            total += match
            q += 1
        elif op == OP_MISMATCH:
            total += mismatch
            q += 1
        else:
            r = q
            while r < n and ops[r] == op:
                r += 1
            if not (free and (q == 0 or r == n)):
                total -= go + ge * (r - q - 1)
            q = r
    return total


def levenshtein(a, b):
    """the textbook two-row recurrence"""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def best_score_by_enumeration(a, b, match, mismatch, go, ge, free):
    """the best rescore() over EVERY global alignment of a and b (every interleaving of diagonal, ref-gap and query-gap ops)"""
    n, m = len(a), len(b)
    best = [None]

    def walk(i, j, ops):
        if i == n and j == m:
            s = rescore(ops, match, mismatch, go, ge, free)
            if best[0] is None or s > best[0]:
                best[0] = s
            return
        if i < n and j < m:
            walk(i + 1, j + 1, ops + [OP_MATCH if a[i] == b[j] else OP_MISMATCH])
        if i < n:
            walk(i + 1, j, ops + [OP_REF_GAP])
        if j < m:
            walk(i, j + 1, ops + [OP_QUERY_GAP])

    walk(0, 0, [])
    return best[0]
