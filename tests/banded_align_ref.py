"""CPU reference of banded global pairwise alignment with affine gaps, numpy int64, for csrc/wn_bandalign.hip.

`a` is the reference (rows i), `b` the query (columns j), costs in half units as in tests/pairwise_align_ref.py.  Cell (i, j),
0 <= i <= N, 0 <= j <= M, is IN BAND iff lo <= j - i <= hi.

    H, E, F of a cell that is not in band are -inf wherever they are read
    in-band cells with i, j >= 1: the recurrence, candidate order (diag, E, F; replaced only on strictly greater) and tie rule
                                  (opening wins) of pairwise_align_ref
    in-band border cells          the full matrix's values: 0 with free end gaps, else -(go + ge (k - 1)); H[0][0] = 0; E = F = -inf
    end cell                      (N, M); with free end gaps the candidates (N, M), (N, M-1) .. (N, 0), (N-1, M) .. (0, M) in this
                                  order, in-band cells only: the first is taken, a later one replaces it only if strictly greater
    no alignment                  free: lo > M or hi < -N; penalised: (N, M) is not in band
    trace                         pairwise_align_ref's; head and tail end gaps are ops
    edge_hits                     the path cells (the stop cell, then the cell after every op up to the end cell) on diagonal lo or hi

Only the stripe is stored: the newest H, E, F of every diagonal (a cell of step s = i + j reads diagonals d - 1 and d + 1 at step
s - 1 and its own at s - 2, and only the diagonals with the parity of s have a cell at s, so the update is in place) and one
backpointer byte per diagonal and step: O((N + M) width).  tests/test_banded_align_ref.py holds this file to exhaustive
enumeration and to pairwise_align_ref."""
from collections import namedtuple

import numpy as np

from tests.pairwise_align_ref import OP_MATCH, OP_MISMATCH, OP_QUERY_GAP, OP_REF_GAP, border

NEG = -(1 << 40)
POISON = -(1 << 31)                          # the score of a pair without an alignment, in half units

Result = namedtuple("Result", "status score matches mismatches gaps length ops edge_hits")
NONE = Result(0, POISON, 0, 0, 0, 0, np.zeros(0, dtype=np.uint8), 0)


def in_band(i, j, lo, hi):
    return lo <= j - i <= hi


def has_alignment(n, m, lo, hi, free):
    return (lo <= m and hi >= -n) if free else in_band(n, m, lo, hi)


def align(a, b, lo, hi, match, mismatch, go, ge, free):
    """one pair under the stripe [lo, hi] (lo <= hi) -> Result; NONE when there is no alignment"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n, m = len(a), len(b)
    assert lo <= hi
    if not has_alignment(n, m, lo, hi, free):
        return NONE
    l, h = max(lo, -n), min(hi, m)                                   # the diagonals that meet the rectangle
    w = h - l + 1
    # index x + 1 holds diagonal l + x; 0 and w + 1 are the cells out of band
    H, E, F = (np.full(w + 2, NEG, dtype=np.int64) for _ in range(3))
    bp = np.zeros((n + m + 1, w), dtype=np.uint8)
    for s in range(n + m + 1):
        x = np.arange((s - l) & 1, w, 2)
        d = l + x
        i, j = (s - d) // 2, (s + d) // 2
        x, i, j = (v[(i >= 0) & (j >= 0) & (i <= n) & (j <= m)] for v in (x, i, j))
        if len(x) == 0:
            continue
        edge = (i == 0) | (j == 0)
        xb, kb = x[edge], np.maximum(i[edge], j[edge])
        x, i, j = x[~edge], i[~edge], j[~edge]
        eo, ee = H[x] - go, E[x] - ge                                # diagonal d - 1 at step s - 1: cell (i, j - 1)
        fo, fe = H[x + 2] - go, F[x + 2] - ge                        # diagonal d + 1 at step s - 1: cell (i - 1, j)
        e, f = np.maximum(eo, ee), np.maximum(fo, fe)
        hh = H[x + 1] + np.where(a[i - 1] == b[j - 1], match, mismatch)      # its own at step s - 2: cell (i - 1, j - 1)
        k = np.zeros(len(x), dtype=np.uint8)
        pick = e > hh
        hh = np.where(pick, e, hh)
        k[pick] = 1
        pick = f > hh
        hh = np.where(pick, f, hh)
        k[pick] = 2
        H[x + 1], E[x + 1], F[x + 1] = hh, e, f
        bp[s, x] = k | ((ee > eo).astype(np.uint8) << 2) | ((fe > fo).astype(np.uint8) << 3)
        H[xb + 1] = 0 if free else np.where(kb == 0, 0, -(go + ge * (kb - 1)))
    # every diagonal's newest cell is its last: on the last row or the last column
    cand = [(n, m)]
    if free:
        cand += [(n, j) for j in range(m - 1, -1, -1)] + [(i, m) for i in range(n - 1, -1, -1)]
    best = None
    for i, j in cand:
        if in_band(i, j, lo, hi):
            v = int(H[j - i - l + 1])
            if best is None or v > best[0]:
                best = (v, i, j)
    score, i, j = best
    on_edge = lambda i, j: int(j - i == lo or j - i == hi)           # noqa: E731
    hits = on_edge(i, j)
    back = [OP_REF_GAP] * (n - i) + [OP_QUERY_GAP] * (m - j)
    st = 0
    while i > 0 and j > 0:
        v = int(bp[i + j, j - i - l])
        if st == 0:
            st = v & 3
            if st != 0:
                continue
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
        assert in_band(i, j, lo, hi)
        hits += on_edge(i, j)
    back += [OP_REF_GAP] * i + [OP_QUERY_GAP] * j
    ops = np.array(back[::-1], dtype=np.uint8)
    nm, nx = int((ops == OP_MATCH).sum()), int((ops == OP_MISMATCH).sum())
    return Result(1, score, nm, nx, len(ops) - nm - nx, len(ops), ops, hits)


def path_cells(ops, free):
    """the cells of the path an op row spells: with h the leading run of one gap kind and t the row's length less, with free end
    gaps, its trailing run of one gap kind, the cell before column h and the cell after every column in [h, t)"""
    ops = [int(v) for v in ops]
    n = len(ops)
    h = 0
    while h < n and ops[0] in (OP_REF_GAP, OP_QUERY_GAP) and ops[h] == ops[0]:
        h += 1
    t = n
    if free:
        while t > h and ops[n - 1] in (OP_REF_GAP, OP_QUERY_GAP) and ops[t - 1] == ops[n - 1]:
            t -= 1
    i = j = 0
    cells = []
    for q, op in enumerate(ops[:t]):
        if q == h:
            cells.append((i, j))
        i += op != OP_QUERY_GAP
        j += op != OP_REF_GAP
        if q >= h:
            cells.append((i, j))
    if t == h:
        cells.append((i, j))
    return cells


def clamp_band(lo, hi, max_band):
    """[lo, hi] about its centre to at most max_band diagonals"""
    if max_band is not None and hi - lo + 1 > max_band:
        lo = lo + (hi - lo + 1 - max_band) // 2
        hi = lo + max_band - 1
    return lo, hi


def band_from_ops(ops, margin=0, max_band=None, free=True):
    """the stripe of the path of an op row, widened by margin on each side, clamped about its centre to max_band"""
    d = [j - i for i, j in path_cells(ops, free)]
    return clamp_band(min(d) - margin, max(d) + margin, max_band)
