"""CPU reference of the pileup, the consensus calling rules, the emit and the variant records (csrc/wn_pileup.hip,
wavenet_speech_amd/pileup.py), as plain loops over Python integers, written from the definitions and not from
the kernel: every read is walked in READ orientation and its columns are mapped to the forward strand one by one, insertion runs
are collected whole and turned round for a reverse-strand read.

Labels 1..4 = A, G, C, T, the complement of v is 5 - v.  Ops: 1 match, 2 mismatch, 3 reference label against a gap, 4 query label
against a gap.  tests/test_pileup_ref.py holds this file to hand-worked piles, to strand symmetry and to the planted runs."""
from collections import namedtuple

import numpy as np

LOW_DEPTH, AMBIGUOUS, SUBSTITUTION, DELETION, INSERTION = 1, 2, 4, 8, 16
DEL, OTHER = 4, 5

Pile = namedtuple("Pile", "counts ins_lengths ins_bases used bad")
Calls = namedtuple("Calls", "call ins_len ins_bases flags alt_count offsets consensus")


def empty_pile(R, max_ins):
    return (np.zeros((R, 2, 6), dtype=np.int64), np.zeros((R, max_ins + 1), dtype=np.int64), np.zeros((R, max_ins, 4), dtype=np.int64))


def read_state(ops, ops_len, max_ops, lo, n_ref, strand, n_query, M, R, qual, keep):
    """0 skipped, -1 bad, 1 to be added (it may still lack an aligned column)"""
    if strand < 0 or n_ref == 0 or not keep:
        return 0
    if strand > 1 or n_ref < 0 or lo < 0 or lo + n_ref > R or not 0 <= n_query <= M or not 0 <= ops_len <= max_ops:
        return -1
    row = [int(v) for v in ops[:ops_len]]
    if any(v < 1 or v > 4 for v in row):
        return -1
    if sum(v != 4 for v in row) != n_ref or sum(v != 3 for v in row) != n_query:
        return -1
    if qual is not None and any(int(v) > 93 for v in qual[:n_query]):
        return -1
    return 1


def add_read(tables, ops, lo, n_ref, strand, query, qual, min_qual, max_ins):
    """one valid read into (counts, ins_lengths, ins_bases); False if it has no aligned column"""
    counts, ins_lengths, ins_bases = tables
    row = [int(v) for v in ops]
    aligned = [c for c, v in enumerate(row) if v <= 2]
    if not aligned:
        return False
    first, last = aligned[0], aligned[-1]

    def forward_base(j):
        """0..3, or None for `other`"""
        v = int(query[j])
        if v < 1 or v > 4 or (qual is not None and int(qual[j]) < min_qual):
            return None
        return (5 - v if strand else v) - 1

    i = sum(v != 4 for v in row[:first])
    j = sum(v != 3 for v in row[:first])
    c = first
    while c <= last:
        op = row[c]
        pos = lo + n_ref - 1 - i if strand else lo + i
        if op <= 2:
            base = forward_base(j)
            counts[pos, strand, OTHER if base is None else base] += 1
            i, j, c = i + 1, j + 1, c + 1
        elif op == 3:
            counts[pos, strand, DEL] += 1
            i, c = i + 1, c + 1
        else:
            e = c
            while row[e] == 4:                                       # ends at or before `last`, which is aligned
                e += 1
            run = [forward_base(j + t) for t in range(e - c)]
            if strand:
                run = run[::-1]
            # in read orientation the run lies between reference indices i - 1 and i
            after = lo + n_ref - 1 - i if strand else lo + i - 1
            ins_lengths[after, min(len(run), max_ins + 1) - 1] += 1
            for k, base in enumerate(run[:max_ins]):
                if base is not None:
                    ins_bases[after, k, base] += 1
            j, c = j + (e - c), e
    return True


def pileup_ref(ops, ops_len, lo, ref_lengths, strand, query, query_lengths, R, qual=None, min_qual=0, max_ins=4, keep=None, into=None):
    """ops [B][max_ops], query [B][M] (and qual) as nested sequences or arrays -> Pile (tables int64, used [B], bad: the count)"""
    B = len(ops_len)
    max_ops = len(ops[0]) if B else 0
    M = len(query[0]) if B else 0
    tables = empty_pile(R, max_ins) if into is None else tuple(t.copy() for t in into[:3])
    used, bad = [], 0
    for b in range(B):
        q = None if qual is None else qual[b]
        state = read_state(ops[b], int(ops_len[b]), max_ops, int(lo[b]), int(ref_lengths[b]), int(strand[b]), int(query_lengths[b]), M, R, q,
                           True if keep is None else bool(keep[b]))
        if state == 1:
            state = 1 if add_read(tables, ops[b][:int(ops_len[b])], int(lo[b]), int(ref_lengths[b]), int(strand[b]), query[b], q, min_qual,
                                  max_ins) else 0
        bad += state == -1
        used.append(state)
    return Pile(tables[0], tables[1], tables[2], np.array(used, dtype=np.int8), bad)


def call_position(counts, ins_lengths, ins_bases, r, min_depth, num, den):
    """counts [2][6], ins_lengths [max_ins + 1], ins_bases [max_ins][4] of one position with reference label r ->
    (call, inserted labels, flags, (alt forward, alt reverse))"""
    max_ins = len(ins_lengths) - 1
    c = [int(counts[0][k]) + int(counts[1][k]) for k in range(5)]
    d = sum(c)
    r = min(max(int(r), 0), 255)
    flags, call, called = 0, r, (r - 1 if 1 <= r <= 4 else None)
    if d < min_depth:
        flags |= LOW_DEPTH
    else:
        order = sorted(range(5), key=lambda k: (-c[k], 0 if k == r - 1 and k < 4 else 1, k))
        k = order[0]
        if c[k] * den > num * d:
            called = k
            call = 0 if k == DEL else k + 1
            if k == DEL:
                flags |= DELETION
            elif call != r:
                flags |= SUBSTITUTION
        else:
            flags |= AMBIGUOUS
    alt = (0, 0) if called is None else (int(counts[0][called]), int(counts[1][called]))
    inserted = []
    n = sum(int(v) for v in ins_lengths)
    if d >= min_depth and n * den > num * d:
        fullest = max(range(max_ins + 1), key=lambda l: (int(ins_lengths[l]), -l))
        length = min(fullest + 1, max_ins)
        for k in range(length):
            slot = [int(v) for v in ins_bases[k]]
            if max(slot) == 0:
                break
            inserted.append(1 + max(range(4), key=lambda q: (slot[q], -q)))
    if inserted:
        flags |= INSERTION
    return call, inserted, flags, alt


def call_consensus_ref(pile, reference, min_depth=3, num=1, den=2):
    R = len(reference)
    max_ins = pile.ins_lengths.shape[1] - 1
    call, ins_len, flags = (np.zeros(R, dtype=np.uint8) for _ in range(3))
    ins = np.zeros((R, max_ins), dtype=np.uint8)
    alt = np.zeros((R, 2), dtype=np.int64)
    offsets, consensus = [0], []
    for p in range(R):
        label, inserted, f, a = call_position(pile.counts[p], pile.ins_lengths[p], pile.ins_bases[p], reference[p], min_depth, num, den)
        call[p], ins_len[p], flags[p], alt[p] = label, len(inserted), f, a
        ins[p, :len(inserted)] = inserted
        consensus += ([label] if label != 0 else []) + inserted
        offsets.append(len(consensus))
    return Calls(call, ins_len, ins, flags, alt, np.array(offsets, dtype=np.int64), np.array(consensus, dtype=np.int64))


def variants_ref(reference, calls, pile):
    """[(pos, kind, ref labels, alt labels, depth, alt count, forward, reverse)] sorted by (pos, sub < del < ins)"""
    R = len(reference)
    ref = [int(v) for v in reference]
    depth = pile.counts[:, :, :5].sum((1, 2))
    out, p = [], 0
    while p < R:
        f = int(calls.flags[p])
        a = (int(calls.alt_count[p][0]), int(calls.alt_count[p][1]))
        if f & SUBSTITUTION:
            out.append((p, "sub", (ref[p],), (int(calls.call[p]),), int(depth[p]), a[0] + a[1], a[0], a[1]))
        if f & DELETION and not (p > 0 and int(calls.flags[p - 1]) & DELETION):
            e = p
            while e < R and int(calls.flags[e]) & DELETION:
                e += 1
            gone = tuple(ref[p:e])
            if p > 0:
                rec = (p - 1, "del", (ref[p - 1],) + gone, (ref[p - 1],))
            elif e < R:
                rec = (0, "del", gone + (ref[e],), (ref[e],))
            else:
                rec = (0, "del", gone, ())
            out.append(rec + (int(depth[p]), a[0] + a[1], a[0], a[1]))
        if f & INSERTION:
            n = int(calls.ins_len[p])
            out.append((p, "ins", (ref[p],), (ref[p],) + tuple(int(v) for v in calls.ins_bases[p][:n]), int(depth[p]),
                        int(pile.ins_lengths[p].sum()), None, None))
        p += 1
    out.sort(key=lambda v: (v[0], ("sub", "del", "ins").index(v[1])))
    return out
