"""The inputs that tests/test_genotype_ref.py (CPU) and tests/test_gpu_genotype.py share, each built once: the planted DIPLOID run.
The reference and the twelve records are tests/pileup_cases.py _plant's.  Records at even index are HETEROZYGOUS: haplotype A carries
all twelve, haplotype B only those at odd index.  128 reads of 300 to 500 bases; read b is drawn from haplotype (b >> 1) & 1 on
strand b & 1; reads 0..3 start at the haplotype's first base and reads 4..7 end at its last, the rest are spread evenly with a jitter.
Two variants: error-free reads with qual 25 on every base, and reads with 2 % random substitutions whose wrong bases carry qual 7 and
all others 25.

The seeds are CONDITIONS, not measurements: they are chosen so that the host chain alone (tests/pairwise_align_ref.py ops on the
planted windows, tests/leftalign_ref.py, tests/pileup_ref.py, tests/genotype_ref.py) returns exactly the twelve planted records with
the planted GT in both variants and reference/reference everywhere else (tests/test_genotype_ref.py asserts it)."""
import functools

import numpy as np

from tests import genotype_ref as G
from tests import leftalign_ref as L
from tests import pairwise_align_ref as A
from tests import pileup_cases as C
from tests import pileup_ref as P

PLANT_SEED = 0
NOISE_SEED = 0
READS = 128
PINNED = 4
Q_GOOD, Q_WRONG = 25, 7
MIN_QUAL = 0
SCALE = 100
ALT_PRIOR = 30 * SCALE


def apply_records(ref, records):
    """the haplotype that carries `records` (pileup_cases records), and the reference position of every base of it (an inserted base
    has its predecessor's)"""
    seq, origin, at = [], [], 0
    for pos, kind, ref_labels, alt_labels in records:
        if kind == "sub":
            seq += ref[at:pos] + [alt_labels[0]]
            origin += list(range(at, pos + 1))
            at = pos + 1
        elif kind == "del":                                          # anchored on pos: ref[pos + 1 : pos + len(ref_labels)] goes
            seq += ref[at:pos + 1]
            origin += list(range(at, pos + 1))
            at = pos + len(ref_labels)
        else:
            seq += ref[at:pos + 1] + list(alt_labels[1:])
            origin += list(range(at, pos + 1)) + [pos] * (len(alt_labels) - 1)
            at = pos + 1
    seq += ref[at:]
    origin += list(range(at, len(ref)))
    return seq, origin


@functools.lru_cache(maxsize=None)
def diploid(noisy=False):
    """dict: ref, records [(pos, kind, ref labels, alts, gt)] as genotype_ref.records_ref writes their first five fields, reads,
    strand, window [(lo, length)], labels, lengths, qual [B, M] uint8"""
    rng = np.random.default_rng(PLANT_SEED)
    ref, sample, _, records = C._plant(rng)
    haplotypes = [apply_records(ref, records), apply_records(ref, records[1::2])]
    assert haplotypes[0][0] == sample
    noise = np.random.default_rng(NOISE_SEED)
    reads, quals, strand, window = [], [], [], []
    for b in range(READS):
        seq, origin = haplotypes[(b >> 1) & 1]
        S, n = len(seq), int(rng.integers(300, 501))
        if b < PINNED:
            start = 0
        elif b < 2 * PINNED:
            start = S - n
        else:
            start = int(round((b - 2 * PINNED) * (S - 500) / (READS - 2 * PINNED - 1))) + int(rng.integers(-10, 11))
            start = min(max(start, 0), S - n)
        read, q = list(seq[start:start + n]), [Q_GOOD] * n
        if noisy:
            for t in range(n):
                if noise.random() < C.NOISE:
                    read[t] = (read[t] - 1 + int(noise.integers(1, 4))) % 4 + 1
                    q[t] = Q_WRONG
        strand.append(b & 1)
        reads.append(C.revcomp(read) if b & 1 else read)
        quals.append(q[::-1] if b & 1 else q)
        lo, hi = max(origin[start] - C.PLANT_FLANK, 0), min(origin[start + n - 1] + 1 + C.PLANT_FLANK, C.PLANT_REF)
        window.append((lo, hi - lo))
    labels, lengths = C.rows(reads)
    qual = C.rows(quals, width=labels.shape[1], dtype=np.uint8)[0]
    want = [(pos, kind, ref_labels, (alt_labels,), "0/1" if k % 2 == 0 else "1/1") for k, (pos, kind, ref_labels, alt_labels) in enumerate(records)]
    return dict(ref=ref, records=want, reads=reads, strand=strand, window=window, labels=labels, lengths=lengths, qual=qual)


@functools.lru_cache(maxsize=None)
def weights():
    return G.weights(SCALE)


@functools.lru_cache(maxsize=None)
def diploid_host(noisy=False):
    """the host chain on the planted windows: dict ops, ops_len (left-aligned), pile, evidence, calls, records"""
    run = diploid(noisy)
    refs = [C.window_labels(run["ref"], lo, n, s) for (lo, n), s in zip(run["window"], run["strand"])]
    ops = [L.left_align_row(A.align(a, read).ops, a, read, s)[0] for a, s, read in zip(refs, run["strand"], run["reads"])]
    ops_rows, ops_len = C.rows([list(o) for o in ops], dtype=np.uint8)
    args = (ops_rows, ops_len, [w[0] for w in run["window"]], [w[1] for w in run["window"]], run["strand"], run["labels"], run["lengths"],
            C.PLANT_REF)
    pile = P.pileup_ref(*args, qual=run["qual"], min_qual=MIN_QUAL)
    ev = G.evidence_ref(weights(), *args, qual=run["qual"], min_qual=MIN_QUAL)
    calls = G.call_genotypes_ref(pile, ev.evidence, run["ref"], weights(), alt_prior=ALT_PRIOR)
    return dict(ops=ops_rows, ops_len=ops_len, pile=pile, evidence=ev, calls=calls, records=G.records_ref(run["ref"], calls, pile))


# ---- the hand rows of the calling rules (tests/test_genotype_ref.py works them by hand; tests/test_gpu_genotype.py holds the kernel
# to the reference on them) ----------------------------------------------------------------------------------------------------------
HAND_GAP_QUAL, HAND_PRIOR, HAND_MIN_DEPTH = 20, 10, 3


def hand_weights():
    """a table that is zero but for column 20: HOM 1, HET 3, MIS 10 -- the insertion rows read it at gap_qual 20"""
    W = [[0] * 94 for _ in range(3)]
    W[0][20], W[1][20], W[2][20] = 1, 3, 10
    return W


def _row(name, E=None, depth=4, other=0, r=1, ins_lengths=(0, 0, 0), ins_bases=((0,) * 4,) * 2):
    """E: {allele index: (HOM, HET, MIS)}; depth: counts[0][r - 1 or 0], `other` beside it"""
    ev = [[0, 0, 0] for _ in range(5)]
    for k, v in (E or {}).items():
        ev[k] = list(v)
    counts = [[0] * 6, [0] * 6]
    counts[0][0], counts[1][4], counts[0][5] = depth - depth // 2, depth // 2, other
    return dict(name=name, E=ev, counts=counts, r=r, ins_lengths=list(ins_lengths), ins_bases=[list(s) for s in ins_bases])


FULL = ((0, 5, 0, 0), (0, 0, 2, 2))           # slots of an insertion G, then C (ties to the smaller label)
BIG = 2 ** 31
HAND_ROWS = [
    # the tie of reference/reference (index 5 with r = 2) with a heterozygous genotype of smaller index, and one unit off it
    _row("homref_ties_het", {0: (100, 5, 25), 1: (0, 10, 100)}, r=2),
    _row("het_wins_by_one", {0: (100, 4, 25), 1: (0, 10, 100)}, r=2),
    # two heterozygous genotypes tie: the smaller index
    _row("two_hets_tie", {0: (50, 0, 50), 1: (50, 5, 20), 2: (50, 5, 20)}),
    # a base beside the deletion, and the deletion twice
    _row("base_and_deletion", {2: (60, 2, 40), 4: (60, 2, 40)}, r=1),
    _row("ref_and_deletion", {0: (60, 2, 40), 4: (60, 2, 40)}, r=1),
    _row("deleted_twice", {4: (0, 9, 40)}, r=3),
    # min_depth on both sides; `other` is no depth
    _row("depth_2", {1: (0, 9, 40)}, depth=2, other=9),
    _row("depth_3", {1: (0, 9, 40)}, depth=3),
    # r outside 1..4: no prior, no call; a shallow one is LOW_DEPTH first
    _row("r_0", {1: (0, 9, 40)}, r=0), _row("r_7", {1: (0, 9, 40)}, r=7), _row("r_negative", {1: (0, 9, 40)}, r=-3),
    _row("r_300", {1: (0, 9, 40)}, r=300), _row("r_0_shallow", {1: (0, 9, 40)}, r=0, depth=1),
    # the clamps of gq and of qual, on both sides
    _row("gq_at_the_clamp", {0: (0, BIG - 1 - 10, BIG + 5)}), _row("gq_past_the_clamp", {0: (0, BIG - 10, BIG + 5)}),
    _row("qual_at_the_clamp", {0: (7, BIG + 7, BIG - 1 + 7 + 10)}, r=2), _row("qual_past_the_clamp", {0: (7, BIG + 7, BIG + 7 + 10)}, r=2),
    _row("both_far_past", {0: (0, 2 ** 50, 2 ** 51)}, r=4),
    # the insertion: n of d reads show it (weights 1, 3, 10 and the prior 10)
    _row("ins_none", ins_lengths=(0, 0, 0), ins_bases=FULL),
    _row("ins_tie_0_and_1", ins_lengths=(0, 2, 0), ins_bases=FULL),
    _row("ins_one_copy", ins_lengths=(0, 3, 0), ins_bases=FULL),
    _row("ins_two_copies", ins_lengths=(0, 4, 0), ins_bases=FULL),
    _row("ins_more_than_depth", ins_lengths=(1, 2, 2), ins_bases=FULL),
    _row("ins_empty_sequence", ins_lengths=(0, 4, 0), ins_bases=((0,) * 4, (0, 0, 2, 2))),
    _row("ins_short_of_depth", depth=2, ins_lengths=(0, 2, 0), ins_bases=FULL),
    _row("ins_on_a_substituted_site", {0: (100, 4, 25), 1: (0, 10, 100)}, r=2, ins_lengths=(4, 0, 0), ins_bases=FULL),
    _row("ins_beside_r_outside", r=0, ins_lengths=(4, 0, 0), ins_bases=FULL),
]
