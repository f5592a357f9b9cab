"""CPU reference of the realignment against the called haplotypes (csrc/wn_realign.hip, wavenet_speech_amd/realign.py; DESIGN.md
section 7aa), as plain loops over Python integers, written from the definitions and not from the kernels: a haplotype's window is
built position by position in forward order and turned into read orientation as a whole; the two op rows are composed by the
sequential loop of the definition, one op at a time; the score of the result is tests/pairwise_align_ref.py rescore.

Labels 1..4 = A, G, C, T, the complement of v is 5 - v; a called label of 0 is a deleted position.  Op codes are wn_pair_align's: in
the haplotype -> reference row 1 / 2 both, 3 a reference label the haplotype lacks, 4 a haplotype label the reference lacks; in
the read -> haplotype row 1 / 2 both, 3 a haplotype label the read lacks, 4 a read label the haplotype lacks.
tests/test_realign_ref.py holds this file to hand-worked rows and to the planted phased run."""
from collections import namedtuple

import numpy as np

from tests import pairwise_align_ref as A

MAX_INS = 8
POISON = -(1 << 31)                           # wn_pair_align's poisoned score, in half units

HapCalls = namedtuple("HapCalls", "call ins_len ins_bases")          # [H][R], [H][R], [H][R][max_ins] uint8 arrays
Windows = namedtuple("Windows", "labels lengths ops ops_len used bad")
Lifted = namedtuple("Lifted", "score matches mismatches gaps length ops ops_len bad")
Realigned = namedtuple("Realigned", "lifted pick hp delta scores windows alignments")


def haplotype_calls_ref(calls, sites=None, chain=None):
    """calls: a genotype_ref.Calls with sites (phase_ref.Sites) and chain (phase_ref.Chain) -> the two haplotypes; a
    pileup_ref.Calls alone -> the one consensus haplotype"""
    if sites is None:
        call, ins_len, ins_bases = (np.asarray(v, dtype=np.uint8) for v in (calls.call, calls.ins_len, calls.ins_bases))
        return HapCalls(call[None].copy(), ins_len[None].copy(), ins_bases[None].copy())
    R = len(calls.alleles)
    max_ins = np.asarray(calls.ins_bases).shape[1]
    call = np.zeros((2, R), dtype=np.uint8)
    ins_len = np.zeros((2, R), dtype=np.uint8)
    ins_bases = np.zeros((2, R, max_ins), dtype=np.uint8)
    for h in range(2):
        for p in range(R):
            s = sites.site_of[p]
            call[h][p] = int(calls.alleles[p][0]) if s < 0 else sites.alleles[s][chain.parity[s] ^ h]
            if int(calls.ins_copies[p]) == 2:                        # on both haplotypes; one copy lies on neither
                ins_len[h][p] = int(calls.ins_len[p])
                ins_bases[h][p] = calls.ins_bases[p]
    return HapCalls(call, ins_len, ins_bases)


def window_rows(call, ins_len, ins_bases, reference, lo, n, strand, max_ins):
    """one haplotype over [lo, lo + n) in read orientation -> (labels, ops), or None where an ins_len is above max_ins"""
    labels, ops = [], []
    for p in range(lo, lo + n):
        v = int(call[p])
        if v == 0:
            ops.append(3)
        else:
            labels.append(v)
            ops.append(1 if v == int(reference[p]) else 2)
        if p < lo + n - 1:                                           # the insertion after the last position is outside the window
            k = int(ins_len[p])
            if k > max_ins:
                return None
            labels += [int(x) for x in ins_bases[p][:k]]
            ops += [4] * k
        elif int(ins_len[p]) > max_ins:
            return None
    if strand:
        labels = [5 - v if 1 <= v <= 4 else v for v in reversed(labels)]
        ops = ops[::-1]
    return labels, ops


def haplotype_windows_ref(hcalls, reference, lo, ref_lengths, strand, max_hap_ops):
    """-> Windows(labels [H][B][max_hap_ops] int32, lengths [H][B], ops [H][B][max_hap_ops] uint8, ops_len [H][B], used [B] int8, bad);
    a read that is bad on one haplotype is bad on both"""
    H, R = hcalls.call.shape
    max_ins = hcalls.ins_bases.shape[2]
    B = len(lo)
    labels = np.zeros((H, B, max_hap_ops), dtype=np.int32)
    ops = np.zeros((H, B, max_hap_ops), dtype=np.uint8)
    lengths = np.zeros((H, B), dtype=np.int32)
    ops_len = np.zeros((H, B), dtype=np.int32)
    used = np.zeros(B, dtype=np.int8)
    bad = 0
    for b in range(B):
        s, n, at = int(strand[b]), int(ref_lengths[b]), int(lo[b])
        if s < 0 or n == 0:
            continue
        rows = None
        if s <= 1 and at >= 0 and n > 0 and at + n <= R:
            rows = [window_rows(hcalls.call[h], hcalls.ins_len[h], hcalls.ins_bases[h], reference, at, n, s, max_ins) for h in range(H)]
            if any(r is None or len(r[1]) > max_hap_ops for r in rows):
                rows = None
        if rows is None:
            used[b] = -1
            bad += 1
            continue
        used[b] = 1
        for h, (lab, op) in enumerate(rows):
            labels[h][b][:len(lab)] = lab
            ops[h][b][:len(op)] = op
            lengths[h][b], ops_len[h][b] = len(lab), len(op)
    return Windows(labels, lengths, ops, ops_len, used, bad)


def lift_row(a_ops, h_ops, ref, query, hap_len):
    """the composition of A (read against haplotype) and Hh (haplotype against reference): the read against its reference window,
    or None for a bad row"""
    a_ops, h_ops = [int(v) for v in a_ops], [int(v) for v in h_ops]
    if any(v < 1 or v > 4 for v in a_ops + h_ops):
        return None
    out, ia, ih, i, j, k = [], 0, 0, 0, 0, 0
    while True:
        while ih < len(h_ops) and h_ops[ih] == 3:                    # reference labels the haplotype lacks
            out.append(3)
            i, ih = i + 1, ih + 1
        while ia < len(a_ops) and a_ops[ia] == 4:                    # read labels the haplotype lacks: after the 3s of the slot
            out.append(4)
            j, ia = j + 1, ia + 1
        if ia == len(a_ops) and ih == len(h_ops):
            break
        if ia == len(a_ops) or ih == len(h_ops):                     # a haplotype label in one row only
            return None
        a, g = a_ops[ia] <= 2, h_ops[ih] <= 2                        # else 3 in A, 4 in Hh
        ia, ih, k = ia + 1, ih + 1, k + 1
        if a and g:
            if i >= len(ref) or j >= len(query):
                return None
            out.append(1 if int(ref[i]) == int(query[j]) else 2)     # compared afresh
            i, j = i + 1, j + 1
        elif a:
            out.append(4)
            j += 1
        elif g:
            out.append(3)
            i += 1
    if i != len(ref) or j != len(query) or k != hap_len:
        return None
    return out


def lift_ref(a_ops, a_ops_len, windows, pick, ref, ref_lengths, query, query_lengths, max_ops, costs=A.EMBOSS, free=True):
    """a_ops [H][B][.] and a_ops_len [H][B]: wn_pair_align's rows of the read against each haplotype; windows: a Windows; pick [B]
    -> Lifted (score in half units)"""
    H = len(a_ops)
    B = len(pick)
    ops = np.zeros((B, max_ops), dtype=np.uint8)
    ops_len = np.zeros(B, dtype=np.int32)
    stats = np.zeros((B, 5), dtype=np.int64)                         # score, matches, mismatches, gaps, length
    bad = 0
    for b in range(B):
        if int(windows.used[b]) == 0:
            continue
        h = int(pick[b])
        row = None
        n_ref, n_query = int(ref_lengths[b]), int(query_lengths[b])
        if int(windows.used[b]) == 1 and 0 <= h < H and 0 < n_ref <= len(ref[b]) and 0 <= n_query <= len(query[b]):
            n_a, n_h, hap_len = int(a_ops_len[h][b]), int(windows.ops_len[h][b]), int(windows.lengths[h][b])
            if 0 <= n_a <= len(a_ops[h][b]) and 0 <= n_h <= len(windows.ops[h][b]) and 0 <= hap_len <= windows.labels.shape[2]:
                row = lift_row(a_ops[h][b][:n_a], windows.ops[h][b][:n_h], ref[b][:n_ref], query[b][:n_query], hap_len)
        if row is None or len(row) > max_ops:
            stats[b] = [POISON, -1, -1, -1, -1]
            bad += 1
            continue
        ops[b][:len(row)] = row
        ops_len[b] = len(row)
        nm, nx = sum(v == 1 for v in row), sum(v == 2 for v in row)
        stats[b] = [A.rescore(row, *costs, free), nm, nx, len(row) - nm - nx, len(row)]
    return Lifted(stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], stats[:, 4], ops, ops_len, bad)


def picks(scores, used):
    """scores [B][H] -> (pick: the greater score, ties to haplotype 0; hp: 1 / 2, 0 on a tie or a read that is not used; delta)"""
    pick, hp, delta = [], [], []
    for row, u in zip(scores, used):
        second = row[1] if len(row) > 1 else row[0]
        pick.append(1 if second > row[0] else 0)
        hp.append(0 if u != 1 or second == row[0] else 1 + pick[-1])
        delta.append(abs(row[0] - second))
    return pick, hp, delta


def realign_ref(ref_rows, ref_lengths, reads, lo, strand, hcalls, reference, align=None, costs=A.EMBOSS, free=True):
    """the whole step on the host, with the quadratic host aligner unless `align(h, b, haplotype labels, read)` hands in the op row
    of the read against haplotype h (the device's own) -> Realigned"""
    B = len(reads)
    cap = max(1, max(int(n) for n in ref_lengths)) * (1 + hcalls.ins_bases.shape[2])
    windows = haplotype_windows_ref(hcalls, reference, lo, ref_lengths, strand, cap)
    H = hcalls.call.shape[0]
    rows, scores = [[None] * B for _ in range(H)], [[0] * H for _ in range(B)]
    for h in range(H):
        for b in range(B):
            hap = [int(v) for v in windows.labels[h][b][:windows.lengths[h][b]]]
            ops = list(A.align(hap, reads[b], *costs, free).ops) if align is None else list(align(h, b, hap, reads[b]))
            rows[h][b] = ops
            scores[b][h] = A.rescore(ops, *costs, free)
    pick, hp, delta = picks(scores, windows.used)
    width = max(1, max(len(r) for per in rows for r in per))
    a_ops = np.zeros((H, B, width), dtype=np.uint8)
    a_len = np.zeros((H, B), dtype=np.int32)
    for h in range(H):
        for b in range(B):
            a_ops[h][b][:len(rows[h][b])] = rows[h][b]
            a_len[h][b] = len(rows[h][b])
    max_ops = max(int(n) for n in ref_lengths) + max(1, max(len(r) for r in reads))
    lifted = lift_ref(a_ops, a_len, windows, pick, ref_rows, ref_lengths, reads, [len(r) for r in reads], max_ops, costs, free)
    return Realigned(lifted, pick, hp, delta, scores, windows, (a_ops, a_len))
