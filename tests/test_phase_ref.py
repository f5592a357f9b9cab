"""CPU: the reference of the phasing step (tests/phase_ref.py) against values worked by hand -- observations on both strands with cap,
min_qual, flat_qual, a deleted allele, a `neither` base and every read state; links at reach 1 and 8; the chain at every tie; the
phased records -- and the five conditions of the planted run (tests/phase_cases.py), which hold for the host chain alone."""
import numpy as np
import pytest

from tests import genotype_ref as G
from tests import phase_cases as PC
from tests import phase_ref as H
from tests import pileup_cases as C
from tests import pileup_ref as P

SITES, OPS, QUERY, QUAL = PC.SITES, PC.OPS, PC.QUERY, PC.QUAL
CHAIN_LINKS, CHAIN_POS, HAND_CHAIN = PC.CHAIN_LINKS, PC.CHAIN_POS, PC.HAND_CHAIN


def _obs(strand, **kw):
    ops, query, qual = (OPS[::-1], C.revcomp(QUERY), QUAL[::-1]) if strand else (OPS, QUERY, QUAL)
    kw = dict(dict(qual=qual, min_qual=0, flat_qual=20, gap_qual=15, cap=20), **kw)
    return H.observations(SITES, ops, 0, 10, strand, query, kw["qual"], kw["min_qual"], kw["flat_qual"], kw["gap_qual"], kw["cap"])


@pytest.mark.parametrize("strand", [0, 1])
def test_observations_by_hand_on_both_strands(strand):
    # G at 1 is the second allele, capped from 30 to 20; the gap at 3 is the deleted allele at min(15, 20); C at 4 is neither G nor T;
    # A at 6 is the first allele at qual 5; the label 0 at 8 is `other`: no observation
    assert _obs(strand) == [(0, 1, 20), (1, 1, 15), (2, H.NEITHER, 10), (3, 0, 5)]
    assert _obs(strand, min_qual=5) == [(0, 1, 20), (1, 1, 15), (2, H.NEITHER, 10), (3, 0, 5)]     # both sides of min_qual
    assert _obs(strand, min_qual=6) == [(0, 1, 20), (1, 1, 15), (2, H.NEITHER, 10)]
    assert _obs(strand, min_qual=11) == [(0, 1, 20), (1, 1, 15)]                                  # the gap has no qual to fail
    assert _obs(strand, cap=93) == [(0, 1, 30), (1, 1, 15), (2, H.NEITHER, 10), (3, 0, 5)]          # the cap above, at and below q
    assert _obs(strand, cap=10) == [(0, 1, 10), (1, 1, 10), (2, H.NEITHER, 10), (3, 0, 5)]
    assert _obs(strand, cap=4, gap_qual=3) == [(0, 1, 4), (1, 1, 3), (2, H.NEITHER, 4), (3, 0, 4)]
    assert _obs(strand, qual=None, flat_qual=33, min_qual=50, cap=93) == [(0, 1, 33), (1, 1, 15), (2, H.NEITHER, 33), (3, 0, 33)]
    assert _obs(strand, qual=None, flat_qual=33, min_qual=50) == [(0, 1, 20), (1, 1, 15), (2, H.NEITHER, 20), (3, 0, 20)]


def test_end_columns_and_a_read_without_an_aligned_column():
    # the deletion at 1 and the base after the last aligned column are end columns: only position 3 is shown (T: neither of C, deleted)
    assert H.observations(SITES, [3, 3, 1, 1, 3, 4], 0, 5, 0, [1, 4, 2], None, 0, 20, 20, 93) == [(1, H.NEITHER, 20)]
    assert H.observations(SITES, [3, 3, 4], 0, 2, 0, [1], None, 0, 20, 20, 93) is None


def _batch(rows):
    """rows: dicts ops, lo, n_ref, strand, query -> read_observations' positional arguments"""
    ops, ops_len = C.rows([r["ops"] for r in rows], dtype=np.uint8)
    query, q_len = C.rows([r["query"] for r in rows])
    return (ops, [r.get("ops_len", n) for r, n in zip(rows, ops_len)], [r["lo"] for r in rows], [r["n_ref"] for r in rows], [r["strand"] for r in rows],
            query, [r.get("query_len", n) for r, n in zip(rows, q_len)])


def test_every_read_state():
    good = dict(ops=[1, 1, 1], lo=0, n_ref=3, strand=0, query=[1, 2, 3])
    rows = [good, dict(good, strand=-1), dict(good, n_ref=0), dict(good, ops=[3, 3, 3], query=[], query_len=0), dict(good, ops=[1, 5, 1]),
            dict(good, lo=8), dict(good, strand=2), dict(good, query_len=2), dict(good, lo=1)]
    per_read, used, bad = H.read_observations(SITES, *_batch(rows), keep=[True] * 8 + [False])
    assert used.tolist() == [1, 0, 0, 0, -1, -1, -1, -1, 0] and bad == 4
    assert per_read == [[(0, 1, 20)]] + [None] * 8
    assert used.tolist() == P.pileup_ref(*_batch(rows), 10, keep=[True] * 8 + [False]).used.tolist()      # the pileup's states
    links = H.links_ref(SITES, *_batch(rows), keep=[True] * 8 + [False])
    assert links.observed == [[0, 1, 0]] + [[0, 0, 0]] * 4 and links.bad == 4 and not any(v for s in links.links for c in s for v in c)
    bad_qual = H.read_observations(SITES, *_batch([good]), qual=[[3, 94, 3]])
    assert bad_qual[1].tolist() == [-1]


def test_links_by_hand_at_reach_1_and_8():
    reads = _batch([dict(ops=OPS, lo=0, n_ref=10, strand=0, query=QUERY)] * 2)
    kw = dict(qual=[QUAL, QUAL], gap_qual=15, cap=[20, 93])
    # read 0 shows sites 0 (x 1, 20), 1 (x 1, 15) and 3 (x 0, 5); read 1 is uncapped: 30 at site 0; site 2 is neither: no link
    one = H.links_ref(SITES, *reads, reach=1, **kw)
    assert one.links == [[[0, 0]], [[30, 0]], [[0, 0]], [[0, 0]], [[0, 0]]]
    assert one.observed == [[0, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 0], [0, 0, 0]]
    far = H.links_ref(SITES, *reads, reach=8, **kw)
    want = [[[0, 0] for _ in range(8)] for _ in range(5)]
    want[1][0][0] = 30                                               # sites 0 and 1: both second alleles, min(20, 15) + min(30, 15)
    want[3][1][1], want[3][2][1] = 10, 10                            # site 3 against 1 and 0: trans, min(., 5) twice
    assert far.links == want
    again = H.links_ref(SITES, *reads, reach=8, into=far, **kw)      # accumulation doubles everything; `far` is left alone
    assert again.links[1][0][0] == 60 and again.observed[3] == [4, 0, 0] and far.links == want


@pytest.mark.parametrize("reach", [1, 8])
def test_a_read_with_more_sites_than_reach(reach):
    n = reach + 3
    sites = H.Sites(list(range(0, 2 * n, 2)), [(1, 2)] * n, [p // 2 if p % 2 == 0 else -1 for p in range(2 * n)])
    query = [1 + (p // 2) % 2 if p % 2 == 0 else 3 for p in range(2 * n)]      # the alleles alternate: d odd is trans, d even cis
    got = H.links_ref(sites, *_batch([dict(ops=[1] * 2 * n, lo=0, n_ref=2 * n, strand=0, query=query)]), reach=reach, flat_qual=7)
    for s in range(n):
        for d in range(1, reach + 1):
            assert got.links[s][d - 1] == ([0, 0] if d > s else [0, 7] if d % 2 else [7, 0]), (s, d)
    assert sum(v for s in got.links for c in s for v in c) == 7 * sum(n - d for d in range(1, reach + 1))


def test_the_chain_at_every_tie():
    c = H.chain_ref(CHAIN_LINKS, CHAIN_POS, min_margin=1)
    assert c.parent == [0, 0, 1, 3, 3, 3] and c.flip == [0, 0, 1, 0, 1, 1] and c.margin == [0, 3, 4, 0, 1, 2 ** 31 - 1]
    assert c.root == [0, 0, 0, 3, 3, 3] and c.parity == [0, 0, 1, 0, 1, 1] and c.ps == [3, 3, 3, 40, 40, 40] and c.set_size == [3] * 6
    c = H.chain_ref(CHAIN_LINKS, CHAIN_POS, min_margin=2)            # the other side of min_margin for site 4
    assert c.parent == [0, 0, 1, 3, 4, 3] and c.set_size == [3, 3, 3, 2, 1, 2] and c.ps[4] == 41 and c.margin[4] == 0
    c = H.chain_ref(CHAIN_LINKS, CHAIN_POS, min_margin=0)            # cis == trans links site 3 to its nearest neighbour, cis
    assert c.parent == [0, 0, 1, 2, 3, 3] and c.flip[3] == 0 and c.root == [0] * 6 and c.parity == [0, 0, 1, 1, 0, 0] and c.set_size == [6] * 6
    c = H.chain_ref(CHAIN_LINKS, CHAIN_POS, min_margin=5)
    assert c.parent == [0, 1, 2, 3, 4, 3] and c.set_size == [1, 1, 1, 2, 1, 2]
    assert H.chain_ref([], []) == H.Chain([], [], [], [], [], [], [])


def test_haplotags_by_hand():
    chain = H.chain_ref(CHAIN_LINKS[:5], SITES.pos)                  # sets {0, 1, 2} and {3, 4}; parity 0, 0, 1, 0, 1
    assert chain.root == [0, 0, 0, 3, 3] and chain.parity == [0, 0, 1, 0, 1]
    row = lambda query, qual, **kw: dict(dict(ops=[1] * 10, lo=0, n_ref=10, strand=0, query=query, qual=qual), **kw)      # noqa: E731
    rows = [row([4, 1, 4, 3, 4, 4, 1, 4, 3, 4], [9, 20, 9, 20, 30, 9, 30, 9, 5, 9]),   # the tie of 30 at sites 2 and 3 goes to site 2
            row([4, 1, 4, 3, 2, 4, 4, 4, 4, 4], [9, 20, 9, 5, 25, 9, 9, 9, 9, 9]),     # 20 + 5 against 25: hp 0; T at site 3 lies in the other set
            row([4, 4, 4, 4, 3, 4, 2, 4, 2, 4], [9] * 10),                             # only `neither`: no observation counts
            row([4, 1, 4, 4, 4, 4], [9] * 6, ops=[1] * 6, n_ref=6, strand=-1)]
    rows[0]["query"][4] = 4                                          # site 2 shows T: its second allele, on haplotype 1 (parity 1)
    reads = _batch(rows)
    tags = H.haplotag_ref(SITES, chain, *reads, qual=C.rows([r["qual"] for r in rows], dtype=np.uint8)[0])
    # read 0: in the set of site 2: A at 0 (x 0, parity 0 -> haplotype 1, 20), C at 1 (x 0 -> 1, 20), T at 2 (x 1, parity 1 -> 1, 30);
    # in the other set: A at site 3 and C at site 4
    assert tags.hp == [1, 0, 0, 0] and tags.ps == [1, 1, -1, -1]
    assert tags.weight == [[70, 0], [25, 25], [0, 0], [0, 0]] and tags.n_sites == [[3, 2], [3, 1], [0, 0], [0, 0]]
    assert tags.used.tolist() == [1, 1, 1, 0]


def test_phased_records_by_hand():
    ref, calls, pile = PC.hand_calls()
    sites = H.sites_ref(calls.flags, calls.alleles)
    assert sites.pos == [1, 2, 3, 5, 7] and sites.alleles == [(2, 0), (1, 0), (4, 0), (2, 0), (1, 2)] and sites.site_of == [-1, 0, 1, 2, -1, 3, -1, 4]
    got = H.phased_records_ref(ref, calls, pile, sites, HAND_CHAIN)
    assert got == [
        (0, "del", (1, 2), ((2,),), "1/1", 2, 1, 3, None),           # homozygous: no site
        (0, "del", (1, 2, 3, 4), ((1,),), "1|0", 1002, 101, 4, 1),   # first deleted position 1: parity 1, the deletion on haplotype 1
        (2, "sub", (3,), ((1,), ()), "2|1", 2002, 201, 5, 1),        # A beside `*`: parity 1 puts `*` on haplotype 1
        (4, "sub", (1,), ((2,),), "1/1", 4002, 401, 7, None),
        (4, "del", (1, 2), ((1,),), "0/1", 5002, 501, 8, None),      # its site stands alone: unphased
        (4, "ins", (1,), ((1, 4, 1),), "0/1", 47, 45, 7, None),      # insertions are never phased
        (5, "del", (2, 3), ((2,),), "1/1", 6002, 601, 9, None),
        (7, "sub", (4,), ((1,), (2,)), "1|2", 7002, 701, 10, 1)]
    flipped = HAND_CHAIN._replace(parity=[0, 0, 1, 1, 1])
    assert [r[4] for r in H.phased_records_ref(ref, calls, pile, sites, flipped)] == ["1/1", "0|1", "1|2", "1/1", "0/1", "0/1", "1/1", "2|1"]
    alone = HAND_CHAIN._replace(set_size=[1] * 5)
    assert [r[:8] for r in H.phased_records_ref(ref, calls, pile, sites, alone)] == G.records_ref(ref, calls, pile)


@pytest.mark.parametrize("noisy", [False, True])
def test_the_planted_run_meets_its_five_conditions(noisy):
    run, host = PC.planted(noisy), PC.planted_host(noisy)
    n_tagged = PC.check_conditions(run, host)
    assert n_tagged > PC.READS // 2
    stretches = [[p for p in sorted(run["sites"]) if run["stretch"][p] == k] for k in (0, 1)]
    assert stretches[1][0] - stretches[0][-1] > PC.DESERT and all(40 <= b - a <= 90 or b - a == 1 for s in stretches for a, b in zip(s, s[1:]))
    for s in stretches:                                              # the alt lies on A at some sites and on B at others
        assert len({run["sites"][p][0] == run["ref"][p] for p in s}) == 2
    records = host["records"]
    assert sorted((r[0], r[1]) for r in records if r[4] == "1/1") == sorted(run["hom"]) and len(run["hom"]) == 4
    assert [(r[0], r[4], r[8]) for r in records if r[1] == "ins"] == [(p, "0/1", None) for p in sorted(run["ins"])] and len(run["ins"]) == 2
    phased = [r for r in records if r[8] is not None]
    assert len(phased) + 6 == len(records) and {r[8] for r in phased} == {stretches[0][0], stretches[1][0]}
    assert {r[4] for r in phased} == {"0|1", "1|0"}
    assert host["links"].bad == 0 and host["links"].used.tolist() == [1] * PC.READS
