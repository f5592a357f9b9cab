"""CPU reference of the genotype evidence, the diploid calling rules and the genotype records (csrc/wn_genotype.hip,
wavenet_speech_amd/genotype.py), as plain loops over Python integers, written from the definitions and not from
the kernel: every read is walked in READ orientation and its columns are mapped to the forward strand one by one, as
tests/pileup_ref.py add_read does; which reads are skipped or bad is that file's read_state.

Labels 1..4 = A, G, C, T, the complement of v is 5 - v; allele indices 0..3 the bases, 4 the deletion.  W is a table [3][94] of
integers, rows HOM, HET, MIS.  tests/test_genotype_ref.py holds this file to hand-worked rows and to the planted diploid runs."""
import math
from collections import namedtuple

import numpy as np

from tests import pileup_ref as P

LOW_DEPTH, SUBSTITUTION, DELETION, INSERTION, HET_FLAG, INS_HET = 1, 4, 8, 16, 32, 64
HOM, HET, MIS = 0, 1, 2
I32_MAX = 2 ** 31 - 1
GENOTYPES = [(a, b) for a in range(5) for b in range(a, 5)]

Evidence = namedtuple("Evidence", "evidence used bad")
Calls = namedtuple("Calls", "alleles gq qual flags ins_copies ins_len ins_bases ins_gq ins_qual costs")


def weights(scale=100):
    """[3][94] Python integers from the formulas of the issue, in float64"""
    rows = [[], [], []]
    for q in range(94):
        e = min(10.0 ** (-q / 10.0), 0.75)
        rows[HOM].append(round(-10.0 * math.log10(1.0 - e) * scale))
        rows[HET].append(round(-10.0 * math.log10((1.0 - e) / 2.0 + e / 6.0) * scale))
        rows[MIS].append(round(-10.0 * math.log10(e / 3.0) * scale))
    return rows


def add_read(evidence, W, ops, lo, n_ref, strand, query, qual, min_qual, flat_qual, gap_qual, cap):
    """one valid read into evidence [R][5][3]"""
    row = [int(v) for v in ops]
    aligned = [c for c, v in enumerate(row) if v <= 2]
    if not aligned:
        return False
    first, last = aligned[0], aligned[-1]
    i = sum(v != 4 for v in row[:first])
    j = sum(v != 3 for v in row[:first])
    for c in range(first, last + 1):
        op = row[c]
        pos = lo + n_ref - 1 - i if strand else lo + i
        if op <= 2:
            v = int(query[j])
            q = flat_qual if qual is None else int(qual[j])
            if 1 <= v <= 4 and not (qual is not None and q < min_qual):
                k = (5 - v if strand else v) - 1
                for t in range(3):
                    evidence[pos][k][t] += int(W[t][min(q, cap)])
            i, j = i + 1, j + 1
        elif op == 3:
            for t in range(3):
                evidence[pos][4][t] += int(W[t][min(gap_qual, cap)])
            i += 1
        else:
            j += 1
    return True


def evidence_ref(W, ops, ops_len, lo, ref_lengths, strand, query, query_lengths, R, qual=None, flat_qual=20, gap_qual=20, cap=None, min_qual=0,
                 keep=None, into=None):
    """-> Evidence(evidence: nested lists [R][5][3] of Python integers, used [B], bad: the count)"""
    B = len(ops_len)
    max_ops = len(ops[0]) if B else 0
    M = len(query[0]) if B else 0
    evidence = [[[0] * 3 for _ in range(5)] for _ in range(R)] if into is None else [[list(c) for c in p] for p in into]
    used, bad = [], 0
    for b in range(B):
        q = None if qual is None else qual[b]
        state = P.read_state(ops[b], int(ops_len[b]), max_ops, int(lo[b]), int(ref_lengths[b]), int(strand[b]), int(query_lengths[b]), M, R, q,
                             True if keep is None else bool(keep[b]))
        if state == 1:
            state = 1 if add_read(evidence, W, ops[b][:int(ops_len[b])], int(lo[b]), int(ref_lengths[b]), int(strand[b]), query[b], q, min_qual,
                                  flat_qual, gap_qual, 93 if cap is None else int(cap[b])) else 0
        bad += state == -1
        used.append(state)
    return Evidence(evidence, np.array(used, dtype=np.int8), bad)


def genotype_costs(E, r, alt_prior):
    """the 15 costs of one position, E [5][3]; r the clamped reference label"""
    out = []
    for a, b in GENOTYPES:
        if a == b:
            like = int(E[a][HOM]) + sum(int(E[x][MIS]) for x in range(5) if x != a)
        else:
            like = int(E[a][HET]) + int(E[b][HET]) + sum(int(E[x][MIS]) for x in range(5) if x not in (a, b))
        out.append(like + (0 if (a == b == r - 1 or not 1 <= r <= 4) else alt_prior))
    return out


def call_position(E, counts, ins_lengths, ins_bases, r, W, gap_qual, alt_prior, min_depth):
    """-> (alleles (2), gq, qual, flags, ins_copies, inserted labels, ins_gq, ins_qual, costs)"""
    max_ins = len(ins_lengths) - 1
    d = sum(int(counts[s][k]) for s in range(2) for k in range(5))
    r = min(max(int(r), 0), 255)
    costs = genotype_costs(E, r, alt_prior)
    alleles, gq, qual, flags = (r, r), 0, 0, 0
    if d < min_depth:
        flags |= LOW_DEPTH
    elif 1 <= r <= 4:
        order = sorted(range(15), key=lambda g: (costs[g], 0 if GENOTYPES[g] == (r - 1, r - 1) else 1, g))
        a, b = GENOTYPES[order[0]]
        alleles = tuple(0 if x == 4 else x + 1 for x in (a, b))
        gq = min(costs[order[1]] - costs[order[0]], I32_MAX)
        qual = min(costs[GENOTYPES.index((r - 1, r - 1))] - costs[order[0]], I32_MAX)
        if any(x != 0 and x != r for x in alleles):
            flags |= SUBSTITUTION
        if 0 in alleles:
            flags |= DELETION
        if a != b:
            flags |= HET_FLAG
    n = sum(int(v) for v in ins_lengths)
    m = max(d - n, 0)
    hom, het, mis = (int(W[t][gap_qual]) for t in range(3))
    c = [n * mis + m * hom, (n + m) * het + alt_prior, n * hom + m * mis + alt_prior]
    order = sorted(range(3), key=lambda k: (c[k], k))
    copies, inserted, ins_gq, ins_qual = 0, [], 0, 0
    if d >= min_depth:
        copies, ins_gq, ins_qual = order[0], min(c[order[1]] - c[order[0]], I32_MAX), min(c[0] - c[order[0]], I32_MAX)
        if copies >= 1:
            fullest = max(range(max_ins + 1), key=lambda l: (int(ins_lengths[l]), -l))
            for k in range(min(fullest + 1, max_ins)):
                slot = [int(v) for v in ins_bases[k]]
                if max(slot) == 0:
                    break
                inserted.append(1 + max(range(4), key=lambda q: (slot[q], -q)))
            if not inserted:
                copies, ins_gq, ins_qual = 0, 0, 0
    if copies >= 1:
        flags |= INSERTION
    if copies == 1:
        flags |= INS_HET
    return alleles, gq, qual, flags, copies, inserted, ins_gq, ins_qual, costs


def call_genotypes_ref(pile, evidence, reference, W, gap_qual=20, alt_prior=3000, min_depth=3):
    """pile: a pileup_ref Pile (or any object with counts, ins_lengths, ins_bases); evidence [R][5][3] -> Calls of numpy arrays
    (costs as a list of lists of Python integers)"""
    R = len(reference)
    max_ins = len(pile.ins_lengths[0]) - 1
    alleles = np.zeros((R, 2), dtype=np.uint8)
    flags, ins_copies, ins_len = (np.zeros(R, dtype=np.uint8) for _ in range(3))
    gq, qual, ins_gq, ins_qual = (np.zeros(R, dtype=np.int64) for _ in range(4))
    ins = np.zeros((R, max_ins), dtype=np.uint8)
    costs = []
    for p in range(R):
        a, g, q, f, copies, inserted, ig, iq, c = call_position(evidence[p], pile.counts[p], pile.ins_lengths[p], pile.ins_bases[p], reference[p], W,
                                                                gap_qual, alt_prior, min_depth)
        alleles[p], gq[p], qual[p], flags[p], ins_copies[p], ins_len[p], ins_gq[p], ins_qual[p] = a, g, q, f, copies, len(inserted), ig, iq
        ins[p, :len(inserted)] = inserted
        costs.append(c)
    return Calls(alleles, gq, qual, flags, ins_copies, ins_len, ins, ins_gq, ins_qual, costs)


def records_ref(reference, calls, pile):
    """[(pos, kind, ref labels, alts: tuple of label tuples with () for `*`, gt, qual, gq, depth)] sorted by (pos, sub < del < ins)"""
    R = len(reference)
    ref = [int(v) for v in reference]
    depth = [sum(int(pile.counts[p][s][k]) for s in range(2) for k in range(5)) for p in range(R)]
    deleted = lambda p: 0 <= p < R and bool(int(calls.flags[p]) & DELETION)                           # noqa: E731
    hom = lambda p: int(calls.alleles[p][0]) == 0                                                     # noqa: E731
    out = []
    for p in range(R):
        f = int(calls.flags[p])
        a = [int(v) for v in calls.alleles[p]]
        common = (int(calls.qual[p]), int(calls.gq[p]), depth[p])
        if f & SUBSTITUTION:
            bases = [v for v in a if v != 0 and v != ref[p]]
            alts = [(bases[0],)] + [(v,) for v in bases[1:] if v != bases[0]]
            if f & DELETION:
                alts, gt = alts + [()], "1/2"
            elif len(alts) == 2:
                gt = "1/2"
            else:
                gt = "1/1" if len(bases) == 2 else "0/1"
            out.append((p, "sub", (ref[p],), tuple(alts), gt) + common)
        if f & DELETION and not (deleted(p - 1) and hom(p - 1) == hom(p)):
            e = p + 1
            while deleted(e) and hom(e) == hom(p):
                e += 1
            gone = tuple(ref[p:e])
            gt = "1/1" if hom(p) else "0/1"
            if p > 0:
                out.append((p - 1, "del", (ref[p - 1],) + gone, ((ref[p - 1],),), gt) + common)
            elif e < R:
                out.append((0, "del", gone + (ref[e],), ((ref[e],),), gt) + common)
            else:
                out.append((0, "del", gone, ((),), gt) + common)
        if f & INSERTION:
            n = int(calls.ins_len[p])
            out.append((p, "ins", (ref[p],), ((ref[p],) + tuple(int(v) for v in calls.ins_bases[p][:n]),),
                        "1/1" if int(calls.ins_copies[p]) == 2 else "0/1", int(calls.ins_qual[p]), int(calls.ins_gq[p]), depth[p]))
    out.sort(key=lambda v: (v[0], ("sub", "del", "ins").index(v[1])))
    return out
