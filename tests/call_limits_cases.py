"""The inputs that tests/test_call_limits_ref.py (CPU), tests/test_gpu_genotype_limits.py and tests/test_gpu_phase_limits.py share,
each built once from fixed seeds or by construction, and their references, each computed once: the evidence walk
(pileup_evidence_kernel) and the phasing walks (phase_links_kernel, haplotag_kernel) on the reads of tests/pileup_limits_cases.py
-- the seam grid, whole tiles and waves of one op, the size limits, the batch limit -- with quals, caps and site tables beside them,
and what only these two tools need: rows that lap the 512-entry observation ring of phase_links_kernel, a batch of 65535 reads of
two columns (one column can form no link), and a hand-made chain for haplotag on the longest reads.

Everything here is a CONDITION, not a measurement: tests/test_call_limits_ref.py proves from tests/*_ref.py alone what each case
reaches, so that the GPU files cannot pass vacuously."""
import functools

import numpy as np

from tests import genotype_ref as G
from tests import phase_ref as H
from tests import pileup_limits_cases as L
from tests import pileup_ref as P

MIN_QUAL, GAP_QUAL = 12, 17                   # as the first-round tests of both tools use them
REACH = 8
TABLE = G.weights(100)
UNIT = [[1] * 94 for _ in range(3)]           # every weight 1: the evidence is then a count
RING = 512                                    # entries of the observation ring
SITE_SEED = 0                                 # a CONDITION: 0 meets everything tests/test_call_limits_ref.py asserts and was taken (1, 3 and 5, tried
                                              # beside it, each leave one link cell without an add across the first wrap of the ring)
SEED = {"grid": 201, "whole": 202, "size": 203, "batch": 204, "ring": 205, "pairs": 206}


def reads_of(name, strand=None):
    """the Reads of a case; strand 0 or 1 puts all of them on that strand (the grid, whole tiles and the ring are built on strand 0)"""
    reads = {"grid": L.grid, "whole": L.whole, "size": L.size, "batch": L.batch, "ring": ring, "pairs": pairs}[name]()
    return reads if strand is None else L.on_strand(reads, strand)


def read_args(reads):
    return reads.ops, reads.ops_len, reads.lo, reads.n_ref, reads.strand, reads.query, reads.query_len


@functools.lru_cache(maxsize=None)
def quals(name):
    """seeded qual rows of the query's width in 0..93; the ring's from MIN_QUAL on, so that no base of it is turned away"""
    query = reads_of(name).query
    return np.random.default_rng(SEED[name] + 25).integers(MIN_QUAL if name == "ring" else 0, 94, size=query.shape).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def few_quals(name):
    """three values only: the arg-max of haplotag ties all the time"""
    return (np.random.default_rng(SEED[name] + 50).integers(0, 3, size=reads_of(name).query.shape) * 10).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def caps(name):
    """a cap per read in 0..119: below, among and above the quals"""
    return np.random.default_rng(SEED[name] + 100).integers(0, 120, size=len(reads_of(name).ops_len)).astype(np.uint8)


def rules(name):
    """the keyword arguments every reference and every kernel call of a case gets"""
    return dict(qual=quals(name), cap=caps(name), min_qual=MIN_QUAL, gap_qual=GAP_QUAL, keep=reads_of(name).keep)


# ---- site tables ------------------------------------------------------------------------------------------------------------------

def _sites(pos, R, rng):
    """a Sites at `pos`: random pairs of two different labels of 0..4 in allele order (0, the deletion, last)"""
    S = len(pos)
    a = rng.integers(0, 5, size=S)
    b = (a + rng.integers(1, 5, size=S)) % 5
    first = np.where((a == 0) | ((b != 0) & (b < a)), b, a)
    site_of = np.full(R, -1, dtype=np.int64)
    site_of[pos] = np.arange(S)
    return H.Sites([int(p) for p in pos], [(int(u), int(v)) for u, v in zip(first, a + b - first)], site_of.tolist())


@functools.lru_cache(maxsize=None)
def sites_of(kind, R):
    """kind "dense": every position a site; "every2", "every3": every n-th, so that the site distance is not the position distance;
    "sparse": every position with chance 0.2"""
    rng = np.random.default_rng(SITE_SEED + R + {"dense": 0, "every2": 2, "every3": 3, "sparse": 7}[kind])
    if kind == "sparse":
        return _sites(np.flatnonzero(rng.random(R) < 0.2), R, rng)
    return _sites(np.arange(0, R, 1 if kind == "dense" else int(kind[-1])), R, rng)


# ---- the ring family --------------------------------------------------------------------------------------------------------------

RING_N = (511, 512, 513, 520, 767, 768, 769, 1024, 1025, 1033)      # aligned columns of a plain row
RING_U = range(10)                                                   # leading labels that are no base: the ring index lags the lane by u
RING_PLAIN = len(RING_N) * len(RING_U)
RING_SPRINKLED = 0.15
RING_MAX_INS = 4
RING_LO_STEP, RING_LO_MOD = 7, 61             # windows spread over 61 positions: the rows meet the wraps at different sites
# rows that mix the ops through the wrap; with labels that are all bases the observation index is the reference index
RING_MIXED = ([1] * 505 + [3] * 12 + [2] * 300,                      # a deletion run over observations 505..516
              [1] * 512 + [4] * 9 + [1] * 300,                       # observation 511, nine insertion columns, observation 512
              [2] * 508 + [4] * 9 + [1] * 300,                       # the run crosses walk column 512 instead; observation 512 far behind it
              [1] * 300 + [4] * 5 + [2] * 205 + [3] * 10 + [1] * 3 + [4] * 3 + [1] * 640 + [3] * 9 + [4] * 2 + [2] * 6)   # both wraps, some labels no base


@functools.lru_cache(maxsize=None)
def ring():
    """Reads on strand 0 (use on_strand): RING_PLAIN plain rows, the same rows sprinkled with labels outside 1..4, RING_MIXED and
    RING_MIXED reversed -- on strand 1 it is the reversed rows whose runs lie on the wrap"""
    rng = np.random.default_rng(SEED["ring"])
    strings = [[1] * n for n in RING_N for _ in RING_U]
    queries = [[9] * u + [1 + k % 4 for k in range(n - u)] for n in RING_N for u in RING_U]
    for q in list(queries):
        odd = rng.random(len(q)) < RING_SPRINKLED
        queries.append([int(rng.choice([0, 5, 9])) if o else v for v, o in zip(q, odd)])
    mixed = [list(s) for s in RING_MIXED] + [list(s[::-1]) for s in RING_MIXED]      # and back to front, for the walk of strand 1
    strings = strings * 2 + mixed
    queries += [L._labels(rng, L._count(s, 3), odd=0.1 if k % len(RING_MIXED) == 3 else 0.0) for k, s in enumerate(mixed)]
    B = len(strings)
    return L.pack(strings, queries, [RING_LO_STEP * b % RING_LO_MOD for b in range(B)], [0] * B, RING_MAX_INS)


# ---- a batch at the limit that can form links -------------------------------------------------------------------------------------

PAIRS_ALLELES = ((1, 4), (2, 3), (1, 4))


@functools.lru_cache(maxsize=None)
def pairs():
    """65535 reads of ops [1, 1] on R = 3, lo = (b >> 1) & 1 and strand b & 1 as L.batch() has them, the skipped and bad rows at
    its indices.  On the forward strand a column shows one of its position's two alleles (96 %), another base (2 %) or a label
    outside 1..4 (2 %)"""
    rng = np.random.default_rng(SEED["pairs"])
    B = L.MAX_BATCH
    b = np.arange(B)
    lo, strand = (b >> 1) & 1, b & 1
    position = lo[:, None] + np.arange(2)[None, :]
    alleles = np.asarray(PAIRS_ALLELES)[position]                    # [B, 2 columns, 2 alleles]
    shown = np.take_along_axis(alleles, rng.integers(0, 2, size=(B, 2, 1)), 2)[:, :, 0]
    draw = rng.random((B, 2))
    forward = np.where(draw < 0.96, shown, np.where(draw < 0.98, ((shown - 1) ^ 1) + 1, rng.choice([0, 5, 9], size=(B, 2))))
    off = (forward < 1) | (forward > 4)
    reverse = np.where(off, forward, 5 - forward)[:, ::-1]           # read orientation: complemented, back to front
    query = np.where(strand[:, None] == 1, reverse, forward).astype(np.int32)
    ops = np.ones((B, 2), dtype=np.uint8)
    ops[list(L.BATCH_BAD), 1] = 0
    keep = np.ones(B, dtype=bool)
    keep[list(L.BATCH_SKIPPED)] = False
    two = np.full(B, 2, dtype=np.int32)
    return L.Reads(ops, two, lo.astype(np.int32), two, strand.astype(np.int32), query, two, 3, 1, keep)


def pairs_sites():
    return H.Sites([0, 1, 2], list(PAIRS_ALLELES), [0, 1, 2])


# ---- a chain for haplotag on the longest reads --------------------------------------------------------------------------------------

CHAIN_SET = 7


@functools.lru_cache(maxsize=None)
def hand_chain(kind, R):
    """a consistent Chain over sites_of(kind, R) made by hand: sets of CHAIN_SET neighbouring sites, every member linked to the
    set's first site, a seeded parity.  chain_ref is not used: it walks every site to its root, which is quadratic on the
    path-shaped forests long reads produce, and haplotag reads root, parity, set_size and pos only"""
    pos = sites_of(kind, R).pos
    S = len(pos)
    root = [s - s % CHAIN_SET for s in range(S)]
    bits = np.random.default_rng(R + 11).integers(0, 2, size=S).tolist()
    parity = [0 if r == s else int(v) for s, (r, v) in enumerate(zip(root, bits))]
    size = [min(CHAIN_SET, S - r) for r in root]
    return H.Chain(root, parity, [0 if r == s else 1 for s, r in enumerate(root)], root, parity, [pos[r] for r in root], size)


# ---- the references, each computed once ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def evidence(name, strand=None, unit=False):
    """evidence_ref of a case with its quals, caps, MIN_QUAL and GAP_QUAL; unit: with the table of ones and without quals or
    caps, which is what L.*_pile() counted"""
    reads = reads_of(name, strand)
    if unit:
        return G.evidence_ref(UNIT, *read_args(reads), reads.R, keep=reads.keep)
    return G.evidence_ref(TABLE, *read_args(reads), reads.R, **rules(name))


@functools.lru_cache(maxsize=None)
def links(name, strand=None, kind="dense", reach=REACH, near=True):
    """the Links of a case over sites_of(kind, R): links_near_ref, or with near=False the quadratic definition links_ref"""
    reads = reads_of(name, strand)
    sites = pairs_sites() if name == "pairs" else sites_of(kind, reads.R)
    return (H.links_near_ref if near else H.links_ref)(sites, *read_args(reads), reach=reach, **rules(name))


@functools.lru_cache(maxsize=None)
def observations(name, strand=None, kind="dense"):
    """read_observations of a case: ([per read: sorted (site, x, weight)], used, bad)"""
    reads = reads_of(name, strand)
    return H.read_observations(sites_of(kind, reads.R), *read_args(reads), **rules(name))


@functools.lru_cache(maxsize=None)
def ring_chain(strand):
    """chain_ref on the ring family's own links (reach 8, dense sites)"""
    return H.chain_ref(links("ring", strand, "dense", REACH, False).links, sites_of("dense", ring().R).pos)


@functools.lru_cache(maxsize=None)
def ring_tags(strand):
    """haplotag_ref of the ring family under ring_chain, with quals of three values only and a gap_qual among them"""
    reads = reads_of("ring", strand)
    return H.haplotag_ref(sites_of("dense", reads.R), ring_chain(strand), *read_args(reads), qual=few_quals("ring"), gap_qual=10)


@functools.lru_cache(maxsize=None)
def size_tags():
    """haplotag_ref of the reads at the size limits under hand_chain"""
    reads = reads_of("size")
    return H.haplotag_ref(sites_of("dense", reads.R), hand_chain("dense", reads.R), *read_args(reads), **rules("size"))


# ---- the calls over the pile of the reads at the size limits --------------------------------------------------------------------

SIZE_CALL = dict(gap_qual=GAP_QUAL, alt_prior=3000, min_depth=3)


@functools.lru_cache(maxsize=None)
def size_pile():
    """pileup_ref of the reads at the size limits with the quals and MIN_QUAL of their evidence: the two tables belong together"""
    reads = reads_of("size")
    return P.pileup_ref(*read_args(reads), reads.R, qual=quals("size"), min_qual=MIN_QUAL, max_ins=reads.max_ins, keep=reads.keep)


@functools.lru_cache(maxsize=None)
def size_reference():
    """seeded reference labels 0..5 over the 65540 positions: bases, and labels that are none"""
    return np.random.default_rng(SEED["size"] + 7).integers(0, 6, size=L.SIZE_R)


@functools.lru_cache(maxsize=None)
def size_calls():
    return G.call_genotypes_ref(size_pile(), evidence("size").evidence, size_reference(), TABLE, **SIZE_CALL)


# ---- small reads of one shape for the graph captures and the strided rows ---------------------------------------------------------

SMALL_R, SMALL_WIDTH, SMALL_READS = 257, 300, 12


@functools.lru_cache(maxsize=None)
def small(seed):
    """(Reads, qual rows, caps): SMALL_READS random reads on a reference of SMALL_R = 257 positions, both strands, one of them
    over the whole reference; the arrays have the same shapes whatever the seed, so one set can be copied over another in place"""
    rng = np.random.default_rng(seed)
    strings = [[1] * SMALL_R]
    while len(strings) < SMALL_READS:
        s = [int(v) for v in rng.choice([1, 2, 3, 4], size=int(rng.integers(40, 280)), p=[0.6, 0.2, 0.1, 0.1])]
        if L._count(s, 4) <= SMALL_R and L._count(s, 3) <= SMALL_WIDTH:
            strings.append(s)
    queries = [L._labels(rng, L._count(s, 3)) for s in strings]
    lo = [int(rng.integers(0, SMALL_R - L._count(s, 4) + 1)) for s in strings]
    reads = L.pack(strings, queries, lo, [int(v) for v in rng.integers(0, 2, size=SMALL_READS)], 4, R=SMALL_R, width=SMALL_WIDTH,
                   query_width=SMALL_WIDTH)
    return reads, rng.integers(0, 94, size=reads.query.shape).astype(np.uint8), rng.integers(0, 120, size=SMALL_READS).astype(np.uint8)


def small_rules(seed):
    reads, qual, cap = small(seed)
    return dict(qual=qual, cap=cap, min_qual=MIN_QUAL, gap_qual=GAP_QUAL)
