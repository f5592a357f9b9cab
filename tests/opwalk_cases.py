"""One batch of op rows for the four tools that walk them (pileup, pileup_evidence, left_align, quality_profile; csrc/wn_opscan.h,
DESIGN.md section 7u), built once and shared by tests/test_opwalk_ref.py and tests/test_gpu_opwalk.py: valid rows of 0, 1, 64, 255,
256, 257 and 513 columns on both strands, one row of every bad kind, and the skipped kinds.  Every row is given in READ
orientation; its labels satisfy op 1 / 2, so that a valid row is valid for quality_profile too.  The expected values are the four
host references', computed once."""
import functools
from collections import namedtuple

import numpy as np

from tests import genotype_ref as G
from tests import leftalign_ref as L
from tests import pileup_ref as P
from tests import quality_profile_ref as Q

LENGTHS = (0, 1, 64, 255, 256, 257, 513)
WIDTH = 513                                   # columns of the op rows: three tiles of 256, the last with one column
LABELS = WIDTH + 2                            # columns of the label rows: room for one label too many
R, MAX_INS, MIN_QUAL, CLASSES = 1024, 4, 7, 5

Batch = namedtuple("Batch", "kind ops ops_len lo ref ref_len query query_len strand qual")
# valid: walked by all four; bad: refused by all four; strand_only: refused by the three that take a strand; skipped: not looked at
# by those three (quality_profile takes no strand: such a row is valid there)
VALID, BAD, STRAND_ONLY, SKIPPED = "valid", "bad", "strand_only", "skipped"


def _row(rng, n, only=None):
    """(ops, ref labels, query labels) of n columns in read orientation"""
    ops = [1] if n == 1 else [int(v) for v in rng.choice(only or [1, 1, 1, 1, 1, 2, 2, 3, 4, 4], size=n)]
    ref, query = [], []
    for op in ops:
        a = int(rng.integers(1, 5))
        if op != 4:
            ref.append(a)
        if op != 3:
            query.append(a if op == 1 else a % 4 + 1 if op == 2 else int(rng.integers(1, 5)))
    return ops, ref, query


@functools.lru_cache(maxsize=None)
def batch():
    rng = np.random.default_rng(1717)
    rows = [(VALID, dict(strand=s), _row(rng, n)) for n in LENGTHS for s in (0, 1)]
    for op in (0, 5):
        for at in (0, 256, WIDTH - 1):
            rows.append((BAD, dict(poke=(at, op)), _row(rng, WIDTH)))
    rows.append((BAD, dict(ops_len=WIDTH + 1), _row(rng, WIDTH)))
    rows += [(BAD, dict(ref_len=d), _row(rng, 257)) for d in (1, -1)]
    rows += [(BAD, dict(query_len=d), _row(rng, 257)) for d in (1, -1)]
    rows.append((STRAND_ONLY, dict(strand=2), _row(rng, 257)))
    rows.append((SKIPPED, dict(strand=-1), _row(rng, 257)))
    rows.append((SKIPPED, dict(), _row(rng, 64, only=[4])))          # ref_lengths 0 with columns: insertions only
    B = len(rows)
    ops, ref, query = np.zeros((B, WIDTH), np.uint8), np.zeros((B, LABELS), np.int32), np.zeros((B, LABELS), np.int32)
    qual = np.zeros((B, LABELS), np.uint8)
    ops_len, ref_len, query_len, strand = (np.zeros(B, np.int32) for _ in range(4))
    for b, (kind, change, (o, a, q)) in enumerate(rows):
        ops[b, :len(o)], ref[b, :len(a)], query[b, :len(q)] = o, a, q
        qual[b, :len(q)] = rng.integers(0, 94, size=len(q))
        ops_len[b], ref_len[b], query_len[b] = change.get("ops_len", len(o)), len(a) + change.get("ref_len", 0), len(q) + change.get("query_len", 0)
        strand[b] = change.get("strand", 0)
        if "poke" in change:
            ops[b, change["poke"][0]] = change["poke"][1]
    lo = (3 + 2 * np.arange(B)).astype(np.int32)
    assert int((lo + ref_len).max()) <= R and int(max(ref_len.max(), query_len.max())) <= LABELS
    return Batch(tuple(r[0] for r in rows), ops, ops_len, lo, ref, ref_len, query, query_len, strand, qual)


def rows_of(*kinds):
    return [b for b, k in enumerate(batch().kind) if k in kinds]


@functools.lru_cache(maxsize=None)
def references():
    """(Pile, Evidence, Aligned, the profile's dict) of the batch from the four host references; nothing of them is changed later"""
    t = batch()
    pile = P.pileup_ref(t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query, t.query_len, R, qual=t.qual, min_qual=MIN_QUAL, max_ins=MAX_INS)
    evidence = G.evidence_ref(G.weights(), t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query, t.query_len, R, qual=t.qual, min_qual=MIN_QUAL)
    aligned = L.left_align_ref(t.ops, t.ops_len, t.ref, t.ref_len, t.query, t.query_len, t.strand)
    profile = Q.profile(t.ops, t.ops_len, t.ref, t.ref_len, t.query, t.query_len, qual=t.qual, classes=CLASSES)
    return pile, evidence, aligned, profile
