"""CPU reference of the indel left-alignment (csrc/wn_leftalign.hip, wavenet_speech_amd/leftalign.py), as
plain loops over Python lists, written from the rules and not from the kernel.  A reverse-strand read is handled by MIRRORING the
row and both sequences, running the forward rule and mirroring the result back -- not by the kernel's index arithmetic.

Ops: 1 match, 2 mismatch, 3 reference label against a gap, 4 query label against a gap.  `a` is the window in read orientation
(what pairwise_align took), `b` the read.  Walk orientation is the pileup's: the row as it stands on strand 0, everything read
back to front on strand 1 (no complement: only equality is asked).  In walk orientation, one PASS is:

    first, last   the first and last column with op 1 or 2; i_c / j_c the reference / query index of column c
    run           a maximal stretch [c, c + l) of one gap op v strictly inside (first, last); 3s next to 4s are two runs
    barrier g     the last column before c with op 3 or 4, or `first` if there is none after it;  s_max = c - g - 1
    shift s       with (seq, x) = (a, i_c) for v = 3 and (b, j_c) for v = 4: the largest s <= s_max with
                  seq[x - t] == seq[x - t + l] for all t = 1..s
    rewrite       the run's columns become [c - s, c - s + l); the s aligned columns it passed follow it in their order

All runs of a pass are decided on the pass's input.  Passes repeat until one moves nothing (settled) or max_passes have run.
tests/test_leftalign_ref.py holds this file to hand-worked rows, to an exhaustive set of short rows and to the planted runs."""
from collections import namedtuple

import numpy as np

Aligned = namedtuple("Aligned", "ops passes settled bad")


def one_pass(row, a, b):
    """one pass in walk orientation over a valid row -> (new row, moved)"""
    aligned = [c for c, v in enumerate(row) if v <= 2]
    if not aligned:
        return list(row), False
    first, last = aligned[0], aligned[-1]
    i_at, j_at, i, j = [], [], 0, 0
    for v in row:
        i_at.append(i)
        j_at.append(j)
        i += v != 4
        j += v != 3
    out, moved = list(row), False
    g, c = first, first + 1
    while c < last:
        v = row[c]
        if v <= 2:
            c += 1
            continue
        e = c
        while row[e] == v:                                           # ends before `last`, which is aligned
            e += 1
        l = e - c
        seq, x = (a, i_at[c]) if v == 3 else (b, j_at[c])
        s = 0
        while s < c - g - 1 and seq[x - s - 1] == seq[x - s - 1 + l]:
            s += 1
        if s:
            moved = True
            out[c - s:c - s + l] = [v] * l
            out[c - s + l:c + l] = row[c - s:c]
        g, c = e - 1, e
    return out, moved


def state(row_len, max_ops, n_ref, N, strand, n_query, M, ops):
    """0 skipped, -1 bad, 1 to be walked: the pileup's rules without the window and the qual"""
    if strand < 0 or n_ref == 0:
        return 0
    if strand > 1 or not 0 < n_ref <= N or not 0 <= n_query <= M or not 0 <= row_len <= max_ops:
        return -1
    row = [int(v) for v in ops[:row_len]]
    if any(v < 1 or v > 4 for v in row):
        return -1
    if sum(v != 4 for v in row) != n_ref or sum(v != 3 for v in row) != n_query:
        return -1
    return 1


def left_align_row(row, a, b, strand, max_passes=8):
    """one valid row -> (new row, passes that moved a run, settled 0 / 1)"""
    row, a, b = [int(v) for v in row], list(a), list(b)
    if strand:
        row, a, b = row[::-1], a[::-1], b[::-1]
    passes, settled = 0, 0
    for _ in range(max_passes):
        row, moved = one_pass(row, a, b)
        if not moved:
            settled = 1
            break
        passes += 1
    return (row[::-1] if strand else row), passes, settled


def left_align_ref(ops, ops_len, ref, ref_lengths, query, query_lengths, strand, max_passes=8):
    """ops [B][max_ops], ref [B][N], query [B][M] as nested sequences or arrays -> Aligned(ops uint8 [B][max_ops], passes [B],
    settled [B], bad: the count).  A skipped or bad row is copied unchanged."""
    B = len(ops_len)
    out = np.array(ops, dtype=np.uint8).reshape(B, -1).copy()
    max_ops, N, M = out.shape[1], len(ref[0]) if B else 0, len(query[0]) if B else 0
    passes, settled, bad = [], [], 0
    for r in range(B):
        n, n_ref, n_query = int(ops_len[r]), int(ref_lengths[r]), int(query_lengths[r])
        st = state(n, max_ops, n_ref, N, int(strand[r]), n_query, M, out[r])
        if st == 1:
            row, p, s = left_align_row(out[r, :n], ref[r][:n_ref], query[r][:n_query], int(strand[r]), max_passes)
            out[r, :n] = row
        else:
            p, s = 0, (1 if st == 0 else -1)
            bad += st == -1
        passes.append(p)
        settled.append(s)
    return Aligned(out, np.array(passes, dtype=np.int32), np.array(settled, dtype=np.int8), bad)
