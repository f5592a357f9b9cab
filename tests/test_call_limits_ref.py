"""CPU: what the cases of tests/call_limits_cases.py reach, proved from tests/phase_ref.py, tests/genotype_ref.py,
tests/pileup_limits_cases.py and the op strings alone (the library is never loaded), so that tests/test_gpu_genotype_limits.py and
tests/test_gpu_phase_limits.py cannot pass vacuously.  Every assertion is a CONDITION on the construction: if a case misses one,
the case is changed, not the assertion.  The seam grid is used whole, all 3126 reads of it: nothing is trimmed.

Ring index: phase_links_kernel walks a read in ascending forward position on both strands, in tiles of T = 256 op columns, and
gives the k-th observation of the read the ring slot k mod 512; read_observations returns a read's observations sorted by site, so k
is the index into that list."""
import numpy as np
import pytest

from tests import call_limits_cases as K
from tests import genotype_ref as G
from tests import phase_cases as PC
from tests import phase_ref as H
from tests import pileup_cases as C
from tests import pileup_limits_cases as L

T = L.T


# ---- links_near_ref is links_ref ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reach", [1, 8])
@pytest.mark.parametrize("strand", [0, 1])
def test_the_linear_reference_on_the_ring_family(strand, reach):
    near, full = K.links("ring", strand, "dense", reach, True), K.links("ring", strand, "dense", reach, False)
    assert near.links == full.links and near.observed == full.observed and near.used.tolist() == full.used.tolist() and near.bad == full.bad == 0
    assert sum(v for s in full.links for c in s for v in c) > 0


@pytest.mark.parametrize("strand", [0, 1])
def test_the_linear_reference_on_whole_tiles_of_one_op(strand):
    for kind in ("dense", "every3"):
        near, full = K.links("whole", strand, kind, K.REACH, True), K.links("whole", strand, kind, K.REACH, False)
        assert near.links == full.links and near.observed == full.observed and sum(v for s in full.links for c in s for v in c) > 0


def test_the_linear_reference_on_the_hand_rows():
    ops, ops_len = C.rows([PC.OPS, PC.OPS[::-1]], dtype=np.uint8)
    query, query_len = C.rows([PC.QUERY, C.revcomp(PC.QUERY)])
    qual = C.rows([PC.QUAL, PC.QUAL[::-1]], width=query.shape[1], dtype=np.uint8)[0]
    reads = (ops, ops_len, [0, 0], [10, 10], [0, 1], query, query_len)
    for reach in (1, 2, 3, 8):
        for kw in (dict(qual=qual, gap_qual=15), dict(qual=qual, min_qual=10, cap=[29, 6]), dict(flat_qual=41)):
            near, full = H.links_near_ref(PC.SITES, *reads, reach=reach, **kw), H.links_ref(PC.SITES, *reads, reach=reach, **kw)
            assert near.links == full.links and near.observed == full.observed and near.used.tolist() == full.used.tolist()
    assert H.links_near_ref(PC.SITES, *reads, reach=8, qual=qual, gap_qual=15).links[1][0] == [30, 0]         # the value of tests/test_phase_ref.py
    start = H.links_ref(PC.SITES, *reads, reach=2, flat_qual=3)
    assert H.links_near_ref(PC.SITES, *reads, reach=2, flat_qual=5, into=start).links == H.links_ref(PC.SITES, *reads, reach=2, flat_qual=5, into=start).links


@pytest.mark.parametrize("noisy", [False, True])
def test_the_linear_reference_on_the_planted_runs(noisy):
    run, host = PC.planted(noisy), PC.planted_host(noisy)
    reads = (host["ops"], host["ops_len"], [w[0] for w in run["window"]], [w[1] for w in run["window"]], run["strand"], run["labels"], run["lengths"])
    near = H.links_near_ref(host["sites"], *reads, reach=PC.REACH, qual=run["qual"], min_qual=PC.MIN_QUAL)
    assert near.links == host["links"].links and near.observed == host["links"].observed and sum(v for s in near.links for c in s for v in c) > 0


# ---- the site tables ----------------------------------------------------------------------------------------------------------------

def test_the_site_tables():
    R = K.ring().R
    dense, every2, every3, sparse = (K.sites_of(kind, R) for kind in ("dense", "every2", "every3", "sparse"))
    assert dense.pos == list(range(R)) and every2.pos == list(range(0, R, 2)) and every3.pos == list(range(0, R, 3))
    assert 0.15 * R < len(sparse.pos) < 0.25 * R
    for sites in (dense, every2, every3, sparse):
        assert [sites.site_of[p] for p in sites.pos] == list(range(len(sites.pos))) and sum(s >= 0 for s in sites.site_of) == len(sites.pos)
        assert all(a != b and 0 <= a <= 4 and 0 <= b <= 4 and a != 0 and (b == 0 or a < b) for a, b in sites.alleles)   # allele order, 0 last
        assert {b for _, b in sites.alleles} == {0, 2, 3, 4} and {a for a, _ in sites.alleles} == {1, 2, 3, 4}
    for strand in (0, 1):
        for kind in ("dense", "every3", "sparse"):                   # the first allele, the second and neither are all shown
            observed = K.links("ring", strand, kind, K.REACH).observed
            assert all(sum(o[x] for o in observed) > 100 for x in range(3)), (strand, kind)


# ---- the ring family --------------------------------------------------------------------------------------------------------------

def _tiles(reads, b, sites, obs):
    """the observations of read b per tile of T walk columns, from its op string: a column is an observation if it consumes a
    reference label whose position is a site among `obs` (a read meets a position once)"""
    n, lo, n_ref, strand = int(reads.ops_len[b]), int(reads.lo[b]), int(reads.n_ref[b]), int(reads.strand[b])
    seen = {s for s, _, _ in obs}
    flags, i = [], 0
    for v in reads.ops[b][:n]:
        flags.append(v != 4 and sites.site_of[lo + n_ref - 1 - i if strand else lo + i] in seen)
        i += v != 4
    walk = flags[::-1] if strand else flags                          # ascending forward position either way
    assert sum(walk) == len(obs)
    return [sum(walk[t:t + T]) for t in range(0, n, T)]


def _wrap_pairs(obs, at, reach):
    """the linked pairs (e, d, cis or trans) of a read whose later observation has index k >= at and whose earlier one k - e < at"""
    out = []
    for k in range(at, min(at + reach, len(obs))):
        for e in range(k - at + 1, reach + 1):
            (s, x, _), (s2, x2, _) = obs[k], obs[k - e]
            if 1 <= s - s2 <= reach and x != H.NEITHER and x2 != H.NEITHER:
                out.append((e, s - s2, x ^ x2))
    return out


@pytest.mark.parametrize("strand", [0, 1])
def test_the_ring_family_laps_the_ring(strand):
    reads = K.reads_of("ring", strand)
    sites = K.sites_of("dense", reads.R)
    per_read, used, bad = K.observations("ring", strand)
    B, plain = len(reads.ops_len), K.RING_PLAIN
    assert B == 2 * plain + 2 * len(K.RING_MIXED) == 208 and used.tolist() == [1] * B and bad == 0 and K.RING == 512
    assert int(K.quals("ring").min()) == K.MIN_QUAL and int(K.quals("ring").max()) == 93
    counts = [len(o) for o in per_read]
    # every base of a plain row is an observation: n - u of them, u = b % 10 the labels in front that are no base
    assert counts[:plain] == [n - u for n in K.RING_N for u in K.RING_U]
    assert min(counts[:plain]) == 511 - 9 and max(counts[:plain]) == 1033 > 2 * K.RING
    assert {n - u for n in K.RING_N for u in K.RING_U} >= {511, 512, 513, 1023, 1024, 1025}
    assert all(c < n for c, n in zip(counts[plain:2 * plain], counts[:plain])) and min(counts[plain:2 * plain]) > 400
    every_e, every_cell = set(range(1, K.REACH + 1)), {(d, c) for d in range(1, K.REACH + 1) for c in (0, 1)}
    for rows in (range(plain), range(plain, 2 * plain)):             # the first wrap, 511 -> 0: the plain and the sprinkled rows each
        pairs = [p for b in rows for p in _wrap_pairs(per_read[b], K.RING, K.REACH)]
        assert {e for e, _, _ in pairs} == every_e and {(d, c) for _, d, c in pairs} == every_cell
    # the second wrap is reached by the ten plain rows of more than 1024 observations only: every e, not every cell
    assert {e for b in range(plain) for e, _, _ in _wrap_pairs(per_read[b], 2 * K.RING, K.REACH)} == every_e
    assert sum(c > 2 * K.RING for c in counts[:plain]) == 10 and max(counts[plain:2 * plain]) < 2 * K.RING
    for at in (K.RING, 2 * K.RING):                                  # the look-back of reach 1 crosses both
        assert any(p for b in range(plain) for p in _wrap_pairs(per_read[b], at, 1)), at
    # in a plain row the partner d sites back is d entries back; in a sprinkled row entries are missing between them
    assert all(e == d for b in range(plain) for e, d, _ in _wrap_pairs(per_read[b], K.RING, K.REACH))
    assert any(d > e for b in range(plain, 2 * plain) for e, d, _ in _wrap_pairs(per_read[b], K.RING, K.REACH))
    tiles = [_tiles(reads, b, sites, per_read[b]) for b in range(B)]
    assert any(T in t for t in tiles[:plain]) and max(t[0] for t in tiles[plain:2 * plain]) < T
    # on strand 0 the labels in front that are no base put the ring index behind the lane by 1..9 from the first tile on
    assert strand or {T - t[0] for t in tiles[:plain]} == set(range(10))
    assert max(max(t) for t in tiles) == T and all(len(t) >= 2 for t in tiles)
    # the mixed rows, walked front to back on strand 0 and their reversals on strand 1: the walk meets RING_MIXED itself
    first = 2 * plain + (len(K.RING_MIXED) if strand else 0)
    for k, string in enumerate(K.RING_MIXED):
        row = reads.ops[first + k][:int(reads.ops_len[first + k])].tolist()
        assert (row[::-1] if strand else row) == list(string), k
    # every label of the first three is a base and no qual lies below MIN_QUAL: observation k is reference column k
    assert all(counts[first + k] == int(reads.n_ref[first + k]) == L._count(K.RING_MIXED[k], 4) for k in range(3))
    assert 2 * K.RING < counts[first + 3] < L._count(K.RING_MIXED[3], 4)                           # both wraps, with labels that are no base


def test_the_mixed_rows_put_their_runs_on_the_wrap():
    """on strand 0, by hand: observation k of the first three mixed rows is reference column k"""
    a, b, c = (list(s) for s in K.RING_MIXED[:3])
    assert [v for v in a if v != 4][505:517] == [3] * 12 and 505 < K.RING < 516
    assert b[:K.RING] == [1] * K.RING and b[K.RING:K.RING + 9] == [4] * 9 and b[K.RING + 9] == 1      # observation 511, the run, observation 512
    assert c[508:517] == [4] * 9 and 508 < K.RING < 517                                              # the run spans walk column 512
    d = K.RING_MIXED[3]
    assert {1, 2, 3, 4} == set(d) and L._count(d, 4) > 2 * K.RING


@pytest.mark.parametrize("strand", [0, 1])
def test_the_ring_family_is_tagged(strand):
    chain, tags = K.ring_chain(strand), K.ring_tags(strand)
    assert max(chain.set_size) > 100 and set(tags.hp) >= {1, 2} and max(n[0] + n[1] for n in tags.n_sites) > T
    assert set(np.unique(K.few_quals("ring")).tolist()) == {0, 10, 20} and tags.bad == 0


# ---- the seam grid, whole tiles, the size and batch limits: the evidence ------------------------------------------------------------

def _unit_is_the_pile(evidence, pile):
    counts = pile.counts[:, :, :5].sum(1)                            # [R][5] over both strands
    return evidence == [[[int(c)] * 3 for c in row] for row in counts]


@pytest.mark.parametrize("name,strand", [("grid", 0), ("grid", 1), ("whole", 0), ("whole", 1), ("size", None), ("batch", None)])
def test_the_evidence_cases_follow_the_pileup(name, strand):
    pile = {"grid": L.grid_pile, "whole": L.whole_pile}[name](strand) if strand is not None else {"size": L.size_pile, "batch": L.batch_pile}[name]()
    weighed, unit = K.evidence(name, strand), K.evidence(name, strand, unit=True)
    assert weighed.used.tolist() == pile.used.tolist() == unit.used.tolist() and weighed.bad == pile.bad == unit.bad
    assert _unit_is_the_pile(unit.evidence, pile)                    # two independent references agree cell by cell
    cells = np.asarray(weighed.evidence, dtype=object)
    assert cells[:, :4].sum() > 0 and (name == "batch" or cells[:, 4].sum() > 0)                   # bases, and deletions where the case has any
    quals, caps = K.quals(name), K.caps(name)
    assert quals.shape == K.reads_of(name).query.shape and (quals < K.MIN_QUAL).any() and int(quals.max()) == 93
    assert int(caps.min()) < K.MIN_QUAL or name in ("whole", "size")
    if name == "batch":
        assert [(weighed.used == v).sum() for v in (1, 0, -1)] == [65523, 5, 7] and 0 <= int(caps.min()) < 3 and int(caps.max()) > 93
    if name == "size":
        assert len(weighed.evidence) == L.SIZE_R == 65540


# ---- the size limits: the phasing walks -------------------------------------------------------------------------------------------

def test_the_reads_at_the_size_limits_lap_the_ring_128_times():
    reads = K.reads_of("size")
    per_read, used, bad = K.observations("size")
    assert used.tolist() == [1] * 4 and bad == 0 and reads.R == 65540
    # the first string has two aligned columns and both are observations; the second loses bases below MIN_QUAL and labels that are no base
    assert [len(o) for o in per_read] == [65535, 65535, 63754, 63756] and 65535 // K.RING == 127
    assert all(o[0][0] == int(lo) and o[-1][0] == int(lo) + 65534 for o, lo in zip(per_read[:2], reads.lo[:2]))   # i from 0 to 65534
    near = K.links("size")
    assert sum(1 for s in near.links for c in s if c[0] or c[1]) > 100000 and min(sum(o) for o in near.observed[5:65535]) >= 2
    assert max(v for s in near.links for c in s for v in c) < 4 * 94


def test_the_hand_made_chain_is_consistent_and_tags_the_longest_reads():
    reads = K.reads_of("size")
    sites, chain = K.sites_of("dense", reads.R), K.hand_chain("dense", reads.R)
    S = len(sites.pos)
    assert S == 65540 and all(len(t) == S for t in chain)
    assert all(chain.root[r] == r and chain.parity[r] == 0 for r in set(chain.root))
    assert all(0 <= s - r < K.CHAIN_SET for s, r in enumerate(chain.root))
    assert chain.set_size == [chain.root.count(r) for r in chain.root[:K.CHAIN_SET]] * (S // K.CHAIN_SET) + [S % K.CHAIN_SET] * (S % K.CHAIN_SET)
    assert chain.ps == [sites.pos[r] for r in chain.root] and chain.parent == chain.root and chain.flip == chain.parity
    assert 0.4 * S < sum(chain.parity) < 0.5 * S
    tags = K.size_tags()
    assert set(tags.hp) == {1, 2} and all(n[1] > 60000 * 2 // 5 for n in tags.n_sites) and all(1 <= n[0] <= K.CHAIN_SET for n in tags.n_sites)
    assert tags.used.tolist() == [1] * 4 and all(p >= 0 for p in tags.ps)


# ---- the two-column batch -----------------------------------------------------------------------------------------------------------

def test_the_two_column_batch():
    reads = K.pairs()
    assert len(reads.ops_len) == 65535 == L.MAX_BATCH and reads.R == 3 and reads.ops.shape == (65535, 2)
    assert reads.strand[:4].tolist() == [0, 1, 0, 1] and reads.lo[:4].tolist() == [0, 0, 1, 1]
    want = K.links("pairs", None, "dense", 1)
    pile = L.reference_pile(reads)
    assert want.used.tolist() == pile.used.tolist() and want.bad == pile.bad == len(L.BATCH_BAD) == 7
    assert [(want.used == v).sum() for v in (1, 0, -1)] == [65523, 5, 7]
    assert all(want.used[b] == -1 for b in L.BATCH_BAD) and all(want.used[b] == 0 for b in L.BATCH_SKIPPED)
    labels = reads.query.ravel()
    assert 0.015 < ((labels < 1) | (labels > 4)).mean() < 0.025
    sites = K.pairs_sites()
    per_read = H.read_observations(sites, *K.read_args(reads), **K.rules("pairs"))[0]
    adds = {}
    for obs in per_read:
        if obs and len(obs) == 2 and obs[0][1] != H.NEITHER and obs[1][1] != H.NEITHER:
            cell = (obs[1][0], obs[0][1] ^ obs[1][1])
            adds[cell] = adds.get(cell, 0) + 1
    assert sorted(adds) == [(1, 0), (1, 1), (2, 0), (2, 1)] and min(adds.values()) > 10000
    assert all(v > 0 for o in want.observed for v in o) and all(c[0][0] > 10000 and c[0][1] > 10000 for c in want.links[1:])
    assert want.links[0] == [[0, 0]]


# ---- the calls over the pile of the reads at the size limits --------------------------------------------------------------------

def test_the_calls_over_the_size_limit_pile():
    pile, calls = K.size_pile(), K.size_calls()
    R = len(calls.flags)
    assert R == L.SIZE_R == 65540 and -(-R // T) == 257 and pile.used.tolist() == K.evidence("size").used.tolist() == [1] * 4
    # the pile and the evidence were fed the same columns: a cell of the one is empty exactly where the other's is
    counts = pile.counts[:, :, :5].sum(1)
    assert [[any(c) for c in p] for p in K.evidence("size").evidence] == (counts > 0).tolist()
    flags = set(calls.flags.tolist())
    assert {0, G.LOW_DEPTH, G.DELETION, G.DELETION | G.HET_FLAG, G.SUBSTITUTION | G.HET_FLAG} <= flags
    last = calls.flags[(R // T) * T:]                                # the 257th tile holds 4 positions
    assert len(last) == 4 and set(K.size_reference().tolist()) == set(range(6)) and int(calls.gq.max()) > 0 and int(calls.qual.max()) > 0
    assert len(calls.costs) == R and pile.ins_lengths.sum() > 0


def test_the_small_reads_have_one_shape():
    for seed in (1, 2):
        reads, qual, cap = K.small(seed)
        assert reads.ops.shape == reads.query.shape == qual.shape == (K.SMALL_READS, K.SMALL_WIDTH) and reads.R == K.SMALL_R == T + 1
        assert int(reads.n_ref[0]) == K.SMALL_R and set(reads.strand.tolist()) == {0, 1} and len(K.sites_of("dense", K.SMALL_R).pos) == 257
        want = H.links_ref(K.sites_of("dense", K.SMALL_R), *K.read_args(reads), reach=K.REACH, **K.small_rules(seed))
        assert want.used.tolist() == [1] * K.SMALL_READS and sum(v for s in want.links for c in s for v in c) > 0
    assert not np.array_equal(K.small(1)[0].query, K.small(2)[0].query)
