"""The inputs that tests/test_pileup_ref.py (CPU) and tests/test_gpu_pileup.py share, each built once: the two planted runs of the
issue.  A seeded random reference of 2000 bases; a sample genome made from it with six substitutions, deletions of 1, 2 and 3
bases and insertions of 1, 2 and 4 bases, every edit at least 100 bases from either end and at least 30 from the next, no indel
whose placement is ambiguous (shifting the gap by one position would give the same sequence); 48 error-free reads of 300 to 500
bases drawn from the sample on alternating strands, at least 5 deep between the outermost edits.  The noisy run is the same reads
with 2 % random substitutions.

The seeds are CONDITIONS, not measurements: they are chosen so that the host reference alone (tests/pileup_ref.py on the ops of
tests/pairwise_align_ref.py) returns the sample genome as the consensus and the planted edits as the records, in both runs
(tests/test_pileup_ref.py asserts it)."""
import functools

import numpy as np

from tests import pairwise_align_ref as A
from tests import pileup_ref as P

PLANT_SEED = 7
NOISE_SEED = 0
PLANT_REF = 2000
PLANT_READS = 48
PLANT_FLANK = 8
NOISE = 0.02
EDGE, APART = 100, 30
EDITS = (("sub", 1),) * 6 + (("del", 1), ("del", 2), ("del", 3), ("ins", 1), ("ins", 2), ("ins", 4))


def revcomp(seq):
    return [5 - v if 1 <= v <= 4 else v for v in reversed(seq)]


def rows(seqs, width=None, dtype=np.int32):
    """(rows [B, width] zero-padded, lengths [B] int32)"""
    width = max(1, max(len(s) for s in seqs)) if width is None else width
    out = np.zeros((len(seqs), width), dtype=dtype)
    for b, s in enumerate(seqs):
        out[b, :len(s)] = s
    return out, np.array([len(s) for s in seqs], dtype=np.int32)


def read(ops, rng, odd=0.1, quals=True):
    """(ops, n_ref, query, qual) with random labels, a share `odd` of them outside 1..4, and random quals; without quals none
    are drawn and the tuple ends at the query"""
    n_query = sum(v != 3 for v in ops)
    query = [int(v) if rng.random() >= odd else int(rng.choice([0, 5, 9])) for v in rng.integers(1, 5, size=n_query)]
    head = (list(ops), sum(v != 4 for v in ops), query)
    return head + ([int(v) for v in rng.integers(0, 94, size=n_query)],) if quals else head


def random_ops(rng, n):
    return [int(v) for v in rng.choice([1, 2, 3, 4], size=n, p=[0.6, 0.2, 0.1, 0.1])]


def cols(reads):
    """the reads of read() as their four columns"""
    return [r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads], [r[3] for r in reads]


def random_pile(rng, R, max_ins, top=4):
    counts = rng.integers(0, top, size=(R, 2, 6))
    ins_lengths = rng.integers(0, top, size=(R, max_ins + 1)) * (rng.random((R, 1)) < 0.5)
    ins_bases = rng.integers(0, 3, size=(R, max_ins, 4)) * (rng.random((R, max_ins, 1)) < 0.7)
    return P.Pile(counts.astype(np.int64), ins_lengths.astype(np.int64), ins_bases.astype(np.int64), None, 0)


def _ambiguous(ref, kind, p, n, inserted):
    """a deletion of ref[p:p + n], or an insertion of `inserted` between p and p + 1, that a shift by one position leaves unchanged"""
    if kind == "del":
        return ref[p - 1] == ref[p + n - 1] or ref[p] == ref[p + n]
    return inserted[0] == ref[p + 1] or inserted[-1] == ref[p]


def _plant(rng):
    """reference, sample, origin (the reference position of every sample base; an inserted base has its predecessor's) and the
    records [(pos, kind, ref labels, alt labels)] sorted by position"""
    ref = [int(v) for v in rng.integers(1, 5, size=PLANT_REF)]
    while True:
        sites = sorted(int(v) for v in rng.integers(EDGE, PLANT_REF - EDGE - 4, size=len(EDITS)))
        if all(b - a >= APART + 12 for a, b in zip(sites, sites[1:])):
            break
    order = [EDITS[int(k)] for k in rng.permutation(len(EDITS))]
    edits = []
    for p, (kind, n) in zip(sites, order):
        while True:
            inserted = [int(v) for v in rng.integers(1, 5, size=n)]
            if kind == "sub":
                if inserted[0] != ref[p]:
                    break
            elif not _ambiguous(ref, kind, p, n, inserted):
                break
            else:
                p += 1                                               # at most a few steps: the spacing has 8 to spare
        edits.append((p, kind, n, inserted))
    span = lambda e: e[2] if e[1] == "del" else 1                    # noqa: E731  (reference bases an edit touches)
    assert all(b[0] - (a[0] + span(a)) >= APART for a, b in zip(edits, edits[1:]))
    assert edits[0][0] >= EDGE and edits[-1][0] + span(edits[-1]) <= PLANT_REF - EDGE
    sample, origin, records, at = [], [], [], 0
    for p, kind, n, inserted in edits:
        sample += ref[at:p]
        origin += range(at, p)
        if kind == "sub":
            sample.append(inserted[0])
            origin.append(p)
            records.append((p, "sub", (ref[p],), (inserted[0],)))
            at = p + 1
        elif kind == "del":
            records.append((p - 1, "del", tuple(ref[p - 1:p + n]), (ref[p - 1],)))
            at = p + n
        else:
            sample += [ref[p]] + inserted
            origin += [p] * (n + 1)
            records.append((p, "ins", (ref[p],), (ref[p],) + tuple(inserted)))
            at = p + 1
    sample += ref[at:]
    origin += range(at, PLANT_REF)
    return ref, sample, origin, records


@functools.lru_cache(maxsize=None)
def planted(noisy=False):
    """dict: ref, sample, records, reads (lists of labels as sequenced), strand, window [(lo, length)] (the reference stretch a read
    was drawn from, widened by PLANT_FLANK and clamped), labels, lengths"""
    rng = np.random.default_rng(PLANT_SEED)
    ref, sample, origin, records = _plant(rng)
    S = len(sample)
    spans = []
    for b in range(PLANT_READS):
        n = int(rng.integers(300, 501))
        if b < 6:
            start = 0                                                # the ends are covered on purpose
        elif b < 12:
            start = S - n
        else:
            start = int(round((b - 12) * (S - 500) / (PLANT_READS - 13))) + int(rng.integers(-10, 11))
            start = min(max(start, 0), S - n)
        spans.append((start, start + n))
    rng.shuffle(spans)
    cover = np.zeros(S, dtype=np.int64)
    for s, e in spans:
        cover[s:e] += 1
    first, last = origin.index(records[0][0]), S - 1 - origin[::-1].index(records[-1][0] + len(records[-1][2]) - 1)
    assert cover[first:last + 1].min() >= 5, int(cover[first:last + 1].min())
    noise = np.random.default_rng(NOISE_SEED)
    reads, strand, window = [], [], []
    for b, (s, e) in enumerate(spans):
        seq = list(sample[s:e])
        if noisy:
            for t in range(len(seq)):
                if noise.random() < NOISE:
                    seq[t] = (seq[t] - 1 + int(noise.integers(1, 4))) % 4 + 1
        strand.append(b & 1)
        reads.append(revcomp(seq) if b & 1 else seq)
        lo, hi = max(origin[s] - PLANT_FLANK, 0), min(origin[e - 1] + 1 + PLANT_FLANK, PLANT_REF)
        window.append((lo, hi - lo))
    labels, lengths = rows(reads)
    return dict(ref=ref, sample=sample, records=records, reads=reads, strand=strand, window=window, labels=labels, lengths=lengths)


def window_labels(ref, lo, length, strand):
    """the window in read orientation, as ReadMapping.labels returns it"""
    seq = list(ref[lo:lo + length])
    return revcomp(seq) if strand else seq


@functools.lru_cache(maxsize=None)
def planted_host(noisy=False):
    """the host chain on the planted windows: dict ops (list of arrays), pile, calls, variants"""
    run = planted(noisy)
    ops = [A.align(window_labels(run["ref"], lo, n, s), read).ops for (lo, n), s, read in zip(run["window"], run["strand"], run["reads"])]
    ops_rows, ops_len = rows([list(o) for o in ops], dtype=np.uint8)
    pile = P.pileup_ref(ops_rows, ops_len, [w[0] for w in run["window"]], [w[1] for w in run["window"]], run["strand"], run["labels"],
                        run["lengths"], PLANT_REF)
    calls = P.call_consensus_ref(pile, run["ref"])
    return dict(ops=ops_rows, ops_len=ops_len, pile=pile, calls=calls, variants=P.variants_ref(run["ref"], calls, pile))
