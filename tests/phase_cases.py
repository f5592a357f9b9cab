"""The inputs that tests/test_phase_ref.py (CPU) and tests/test_gpu_phase.py share, each built once: the hand rows of the
observations and the PLANTED PHASED run.

The planted run: a seeded random reference of 3000 bases with two stretches of heterozygous sites -- substitutions and deletions of
1 and 2 bases, 40 to 90 bases from one site to the next, none in a homopolymer or where a shift of the gap gives the same sequence
-- and a desert of 700 bases without any between them: longer than the longest read plus both flanks, so no read can link the
stretches and exactly two phase sets can form.  A drawn bit puts the alt of every site on haplotype A or B (both occur in each
stretch).  Each stretch also holds two homozygous records (on both haplotypes: no sites) and one heterozygous insertion (never
phased), each midway between two sites.  160 reads of 300 to 500 bases; read b is drawn from haplotype (b >> 1) & 1 on strand
b & 1; reads 0..3 start at the haplotype's first base and reads 4..7 end at its last, the rest are spread evenly with a jitter.  Two
variants: error-free reads with qual 25 on every base, and reads with 2 % random substitutions whose wrong bases carry qual 7.

The seeds are CONDITIONS, not measurements: they are chosen so that the host chain alone (tests/pairwise_align_ref.py ops on the
planted windows, tests/leftalign_ref.py, tests/pileup_ref.py, tests/genotype_ref.py, tests/phase_ref.py) meets, in both variants,
the five conditions tests/test_phase_ref.py asserts: the sites are exactly the planted ones; two sets split at the desert; the
parity is the planted bit up to one flip per set; every read with an observation has its haplotype's hp; every other read hp 0.
Seeds tried, in order, with NOISE_SEED 0: PLANT_SEED 0 and 1 (the plant's own assertions fail: a stretch lacks one kind of edit or a
spacing leaves 40..90), 2 (all five hold in both variants: taken)."""
import functools

import numpy as np

from tests import genotype_cases as K
from tests import genotype_ref as G
from tests import leftalign_ref as L
from tests import pairwise_align_ref as A
from tests import phase_ref as H
from tests import pileup_cases as C
from tests import pileup_ref as P

PLANT_SEED = 2
NOISE_SEED = 0
PLANT_REF = 3000
READS = 160
PINNED = 4
DESERT = 700
STRETCHES = ((150, 1050), (None, 2850))       # the second starts DESERT after the last site of the first
REACH = 4
MIN_QUAL = 0


# ---- the hand rows (tests/test_phase_ref.py works them by hand; tests/test_phase_abi.py and tests/test_gpu_phase.py hold the package to
# the same values) --------------------------------------------------------------------------------------------------------------------
# positions 1, 3, 4, 6 and 8 of a reference of 10 are sites; site 1 is a heterozygous deletion
SITES = H.Sites([1, 3, 4, 6, 8], [(1, 2), (3, 0), (2, 4), (1, 4), (1, 3)], [-1, 0, -1, 1, 2, -1, 3, -1, 4, -1])
OPS = [1, 1, 1, 3, 1, 1, 1, 1, 1, 1]                                 # position 3 is deleted in the read
QUERY = [4, 2, 4, 3, 4, 1, 4, 0, 4]                                  # at positions 0, 1, 2, 4, ..., 9; the label at 8 is no base
QUAL = [9, 30, 9, 10, 9, 5, 9, 40, 9]

CHAIN_LINKS = [[[9, 9], [9, 9]],                # site 0 is always a root, whatever its cells hold
               [[5, 2], [0, 0]],                # margin 3, cis
               [[2, 6], [7, 3]],                # margins 4 and 4: the tie goes to d = 1, trans
               [[4, 4], [4, 4]],                # cis == trans at both: margin 0
               [[0, 1], [0, 0]],                # margin 1: at min_margin 1
               [[1, 1], [0, 2 ** 40]]]          # d = 2 wins; the margin is clamped
CHAIN_POS = [3, 10, 11, 40, 41, 90]


def hand_calls():
    """the hand-made case of tests/test_genotype_abi.py as reference tables"""
    ref = [1, 2, 3, 4, 1, 2, 3, 4]
    alleles = [(0, 0), (2, 0), (1, 0), (4, 0), (2, 2), (2, 0), (0, 0), (1, 2)]
    D, S, T, I, IH = G.DELETION, G.SUBSTITUTION, G.HET_FLAG, G.INSERTION, G.INS_HET
    flags = [D, D | T, S | D | T, D | T, S | I | IH, D | T, D, S | T]
    R = len(ref)
    counts = np.zeros((R, 2, 6), dtype=np.int64)
    counts[:, 0, 0] = np.arange(R) + 3
    ins_bases = np.zeros((R, 2), dtype=np.int64)
    ins_bases[4] = [4, 1]
    calls = G.Calls(np.array(alleles), np.arange(R) * 100 + 1, np.arange(R) * 1000 + 2, np.array(flags), np.array([0, 0, 0, 0, 1, 0, 0, 0]),
                    np.array([0, 0, 0, 0, 2, 0, 0, 0]), ins_bases, np.arange(R) * 10 + 5, np.arange(R) * 10 + 7, None)
    return ref, calls, P.Pile(counts, np.zeros((R, 3), dtype=np.int64), np.zeros((R, 2, 4), dtype=np.int64), None, 0)


HAND_CHAIN = H.Chain([0, 0, 1, 3, 1], [0, 0, 1, 0, 1], [0, 5, 5, 0, 5], [0, 0, 0, 3, 0], [1, 1, 0, 0, 0], [1, 1, 1, 5, 1], [4, 4, 4, 1, 4])


# ---- the planted run -------------------------------------------------------------------------------------------------------------

def _clean(ref, kind, p, n, inserted):
    """no homopolymer at p and no ambiguous placement"""
    if kind == "sub":
        return ref[p - 1] != ref[p] != ref[p + 1] and inserted[0] != ref[p]
    if kind == "del":
        return not C._ambiguous(ref, "del", p, n, inserted) and ref[p - 1] != ref[p] and ref[p + n - 1] != ref[p + n]
    return not C._ambiguous(ref, "ins", p, n, inserted) and ref[p] != ref[p + 1]


def _place(rng, ref, kind, n, p):
    """an edit (p, kind, n, labels) at the first clean position from p on"""
    while True:
        inserted = [int(v) for v in rng.integers(1, 5, size=n)]
        if kind == "sub":
            inserted = [(ref[p] - 1 + int(rng.integers(1, 4))) % 4 + 1]
        if _clean(ref, kind, p, n, inserted):
            return (p, kind, n, inserted)
        p += 1


def _plant(rng):
    """reference, [(edit, on A, on B)] sorted by position, and the stretch of every edit"""
    ref = [int(v) for v in rng.integers(1, 5, size=PLANT_REF)]
    edits, stretch_of = [], []
    start = STRETCHES[0][0]
    for k, (_, end) in enumerate(STRETCHES):
        het, p = [], start
        while p < end:
            kind, n = (("sub", 1), ("sub", 1), ("sub", 1), ("del", 1), ("del", 2))[int(rng.integers(0, 5))]
            e = _place(rng, ref, kind, n, p)
            het.append(e)
            p = e[0] + int(rng.integers(42, 87))
        gaps = [b[0] - a[0] for a, b in zip(het, het[1:])]
        assert all(40 <= g <= 90 for g in gaps), gaps
        assert {e[1:3] for e in het} == {("sub", 1), ("del", 1), ("del", 2)}
        bits = [int(v) for v in rng.integers(0, 2, size=len(het))]
        assert 0 < sum(bits) < len(bits)
        planted = [(e, bit == 0, bit == 1) for e, bit in zip(het, bits)]
        wide = [t for t, g in enumerate(gaps) if g >= 64]            # room for an edit midway, 30 clear of either site
        assert len(wide) >= 3
        for t, (kind, n, a, b) in zip(rng.permutation(wide)[:3], (("sub", 1, True, True), ("del", 1, True, True), ("ins", 2, None, None))):
            e = _place(rng, ref, kind, n, het[t][0] + gaps[t] // 2 - 1)
            on_a = bool(rng.integers(0, 2)) if a is None else a
            planted.append((e, on_a, (not on_a) if b is None else b))
        planted.sort(key=lambda v: v[0][0])
        span = lambda e: e[2] if e[1] == "del" else 1                # noqa: E731
        assert all(b[0][0] - (a[0][0] + span(a[0])) >= 25 for a, b in zip(planted, planted[1:]))
        edits += planted
        stretch_of += [k] * len(planted)
        start = het[-1][0] + 2 + DESERT
    assert edits[-1][0][0] + 2 <= PLANT_REF - 100
    return ref, edits, stretch_of


def _record(ref, e):
    """an edit as pileup_cases writes its records"""
    p, kind, n, inserted = e
    if kind == "sub":
        return (p, "sub", (ref[p],), (inserted[0],))
    if kind == "del":
        return (p - 1, "del", tuple(ref[p - 1:p + n]), (ref[p - 1],))
    return (p, "ins", (ref[p],), (ref[p],) + tuple(inserted))


@functools.lru_cache(maxsize=None)
def planted(noisy=False):
    """dict: ref, reads, strand, window [(lo, length)], labels, lengths, qual [B, M] uint8, and the truth: sites {position: (label
    on A, label on B)} (0: deleted), stretch {position: 0 or 1}, hom [(pos, kind)] and ins [pos] of the records that are no sites"""
    rng = np.random.default_rng(PLANT_SEED)
    ref, edits, stretch_of = _plant(rng)
    haplotypes = [K.apply_records(ref, [_record(ref, e) for e, on_a, on_b in edits if (on_a, on_b)[h]]) for h in range(2)]
    sites, stretch, hom, ins = {}, {}, [], []
    for (e, on_a, on_b), k in zip(edits, stretch_of):
        p, kind, n, inserted = e
        if kind == "ins":
            ins.append(p)
        elif on_a and on_b:
            hom.append((_record(ref, e)[0], kind))
        else:
            for t in range(n):
                alt = inserted[0] if kind == "sub" else 0
                sites[p + t] = (alt if on_a else ref[p + t], alt if on_b else ref[p + t])
                stretch[p + t] = k
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
        read, q = list(seq[start:start + n]), [K.Q_GOOD] * n
        if noisy:
            for t in range(n):
                if noise.random() < C.NOISE:
                    read[t] = (read[t] - 1 + int(noise.integers(1, 4))) % 4 + 1
                    q[t] = K.Q_WRONG
        strand.append(b & 1)
        reads.append(C.revcomp(read) if b & 1 else read)
        quals.append(q[::-1] if b & 1 else q)
        lo, hi = max(origin[start] - C.PLANT_FLANK, 0), min(origin[start + n - 1] + 1 + C.PLANT_FLANK, PLANT_REF)
        window.append((lo, hi - lo))
    assert DESERT > 500 + 2 * C.PLANT_FLANK
    labels, lengths = C.rows(reads)
    qual = C.rows(quals, width=labels.shape[1], dtype=np.uint8)[0]
    return dict(ref=ref, reads=reads, strand=strand, window=window, labels=labels, lengths=lengths, qual=qual, sites=sites, stretch=stretch,
                hom=hom, ins=ins)


def phase_all(run, ops_rows, ops_len, lo, ref_lengths, pile, calls):
    """the phasing half of the host chain on given ops and windows: dict sites, links, chain, tags, per_read (the observations of every
    read), records"""
    reads = (ops_rows, ops_len, lo, ref_lengths, run["strand"], run["labels"], run["lengths"])
    sites = H.sites_ref(calls.flags, calls.alleles)
    links = H.links_ref(sites, *reads, reach=REACH, qual=run["qual"], min_qual=MIN_QUAL)
    chain = H.chain_ref(links.links, sites.pos)
    tags = H.haplotag_ref(sites, chain, *reads, qual=run["qual"], min_qual=MIN_QUAL)
    per_read = H.read_observations(sites, *reads, qual=run["qual"], min_qual=MIN_QUAL)[0]
    return dict(sites=sites, links=links, chain=chain, tags=tags, per_read=per_read, records=H.phased_records_ref(run["ref"], calls, pile, sites, chain))


@functools.lru_cache(maxsize=None)
def planted_host(noisy=False):
    """the host chain on the planted windows: dict ops, ops_len (left-aligned), pile, evidence, calls and phase_all's entries"""
    run = planted(noisy)
    refs = [C.window_labels(run["ref"], lo, n, s) for (lo, n), s in zip(run["window"], run["strand"])]
    ops = [L.left_align_row(A.align(a, read).ops, a, read, s)[0] for a, s, read in zip(refs, run["strand"], run["reads"])]
    ops_rows, ops_len = C.rows([list(o) for o in ops], dtype=np.uint8)
    lo, ref_lengths = [w[0] for w in run["window"]], [w[1] for w in run["window"]]
    args = (ops_rows, ops_len, lo, ref_lengths, run["strand"], run["labels"], run["lengths"], PLANT_REF)
    pile = P.pileup_ref(*args, qual=run["qual"], min_qual=MIN_QUAL)
    ev = G.evidence_ref(K.weights(), *args, qual=run["qual"], min_qual=MIN_QUAL)
    calls = G.call_genotypes_ref(pile, ev.evidence, run["ref"], K.weights(), alt_prior=K.ALT_PRIOR)
    return dict(ops=ops_rows, ops_len=ops_len, pile=pile, evidence=ev, calls=calls, **phase_all(run, ops_rows, ops_len, lo, ref_lengths, pile, calls))


def check_conditions(run, got):
    """the five conditions of the planted run on phase_all's dict (or on the same tables from the device, as lists, beside the
    reference's per_read); a_first below: whether haplotype A is the set's haplotype 2"""
    sites, chain, tags = got["sites"], got["chain"], got["tags"]
    truth = run["sites"]
    assert list(sites.pos) == sorted(truth), (list(sites.pos), sorted(truth))                       # 1: exactly the planted sites
    for p, pair in zip(sites.pos, sites.alleles):
        assert set(pair) == set(truth[p]) and len(set(pair)) == 2, (p, pair, truth[p])
    sets = sorted(set(chain.root))
    assert len(sets) == 2 and all(n > 1 for n in chain.set_size)                                    # 2: two sets, split at the desert
    assert [sets.index(r) for r in chain.root] == [run["stretch"][p] for p in sites.pos]
    a_is_first = {}                                                                                 # 3: no switch error
    for s, p in enumerate(sites.pos):
        bit = 0 if sites.alleles[s][0] == truth[p][0] else 1                                        # the index of haplotype A's allele
        a_is_first.setdefault(chain.root[s], set()).add(bit ^ chain.parity[s])
    assert all(len(v) == 1 for v in a_is_first.values()), a_is_first
    n_tagged = 0
    for b, (hp, ps) in enumerate(zip(tags.hp, tags.ps)):                                            # 4 and 5
        if got["per_read"][b]:
            root = chain.root[got["per_read"][b][0][0]]
            (a_first,) = a_is_first[root]
            assert hp == 1 + (((b >> 1) & 1) ^ a_first) and ps == sites.pos[root], (b, hp, ps)
            n_tagged += 1
        else:
            assert hp == 0 and ps == -1, (b, hp, ps)
    assert 0 < n_tagged < READS
    return n_tagged
