"""CPU: the host reference of the genotype evidence and the diploid calls (tests/genotype_ref.py) against the check values of the
weight table, hand-worked evidence on both strands, pileup_ref's counts under a table of ones over every short op string, strand
symmetry, the calling rules by hand at every tie, and the planted diploid runs of tests/genotype_cases.py, whose seeds are chosen
so that the host chain alone returns the twelve planted records with the planted GT."""
import itertools
import math

import numpy as np
import pytest

from tests import genotype_cases as K
from tests import genotype_ref as G
from tests import pileup_cases as C
from tests import pileup_ref as P

OPS = [3, 1, 2, 4, 4, 1, 3, 1, 4]             # end, A, G, insertion of 2, G, deletion, other, end (tests/test_pileup_ref.py)
QUERY = [1, 2, 3, 4, 2, 0, 1]
QUAL = [20, 9, 10, 9, 10, 10, 0]
W = G.weights(100)


def test_weight_table_check_values_and_shape():
    assert len(W) == 3 and all(len(row) == 94 for row in W)
    for q, want in ((0, (602, 602, 602)), (2, (433, 538, 677)), (10, (46, 331, 1477)), (20, (4, 304, 2477)), (30, (0, 301, 3477)),
                    (93, (0, 301, 9777))):
        assert tuple(W[t][q] for t in range(3)) == want, q
    assert all(0 <= v <= 2 ** 20 for row in W for v in row)
    assert all(W[G.HOM][q] >= W[G.HOM][q + 1] and W[G.MIS][q] <= W[G.MIS][q + 1] for q in range(93))
    assert W[G.HOM][2] > W[G.HOM][40] == 0 and W[G.MIS][1] < W[G.MIS][2]
    assert W[G.HET][93] == round(100 * 10 * math.log10(2)) == 301 and all(W[G.HET][q] >= W[G.HET][q + 1] for q in range(93))
    assert all(W[G.HOM][q] == W[G.HET][q] == W[G.MIS][q] == 602 for q in (0, 1))             # e = 3 / 4: a base that says nothing
    assert all(W[G.HOM][q] < W[G.HET][q] < W[G.MIS][q] for q in range(2, 94))
    for scale in (1, 7, 1000, 10699):
        t = G.weights(scale)
        assert t[G.MIS][93] == round(97.7712125471966 * scale) <= 2 ** 20 and t[G.HOM][0] == t[G.MIS][0]


def test_the_package_builds_the_same_table():
    import torch
    import wavenet_speech_amd as WN
    for scale in (1, 100, 10699):
        w = WN.genotype_weights(scale)
        assert w.scale == scale and w.table.dtype == torch.int32 and not w.table.is_cuda and w.table.tolist() == G.weights(scale)


def _one(strand, ops=OPS, query=QUERY, lo=2, n_ref=6, R=10, table=W, **kw):
    for name in ("qual",):
        if kw.get(name) is not None:
            kw = dict(kw, **{name: [kw[name]]})
    return G.evidence_ref(table, [ops], [len(ops)], [lo], [n_ref], [strand], [query], [len(query)], R, **kw)


def _nonzero(ev):
    return {(p, k): tuple(c) for p, row in enumerate(ev.evidence) for k, c in enumerate(row) if any(c)}


def _col(q):
    return tuple(W[t][q] for t in range(3))


def test_hand_worked_evidence_on_both_strands():
    ev = _one(0, qual=QUAL)
    assert ev.used.tolist() == [1] and ev.bad == 0
    assert _nonzero(ev) == {(3, 0): _col(20), (4, 1): _col(9), (5, 1): _col(10), (6, 4): _col(20)}
    # reference index i of the ops is forward position 7 - i; the labels are complemented, the quals stay with their bases
    assert _nonzero(_one(1, qual=QUAL)) == {(6, 3): _col(20), (5, 2): _col(9), (4, 2): _col(10), (3, 4): _col(20)}
    # min_qual sends the base of qual 9 to `other`; the cap does not (it is compared with the uncapped qual) but lowers the weights
    assert _nonzero(_one(0, qual=QUAL, min_qual=10)) == {(3, 0): _col(20), (5, 1): _col(10), (6, 4): _col(20)}
    assert _nonzero(_one(0, qual=QUAL, min_qual=10, cap=[9], gap_qual=30)) == {(3, 0): _col(9), (5, 1): _col(9), (6, 4): _col(9)}
    assert _nonzero(_one(0, qual=QUAL, cap=[10])) == {(3, 0): _col(10), (4, 1): _col(9), (5, 1): _col(10), (6, 4): _col(10)}
    assert _nonzero(_one(0, qual=QUAL, cap=[200], gap_qual=93)) == {(3, 0): _col(20), (4, 1): _col(9), (5, 1): _col(10), (6, 4): _col(93)}
    # no qual: flat_qual on every base, and min_qual asks nothing
    assert _nonzero(_one(1, flat_qual=7, min_qual=50, gap_qual=3)) == {(6, 3): _col(7), (5, 2): _col(7), (4, 2): _col(7), (3, 4): _col(3)}
    for kw, state in ((dict(strand=-1), 0), (dict(n_ref=0), 0), (dict(keep=[False]), 0), (dict(ops=[3] * 6 + [4] * 7), 0), (dict(strand=2), -1),
                      (dict(lo=5), -1), (dict(ops=OPS[:-1] + [5]), -1), (dict(qual=[94] + [0] * 6), -1), (dict(qual=[93] * 7), 1)):
        args = dict(dict(strand=0), **kw)
        ev = _one(args.pop("strand"), **args)
        assert ev.used.tolist() == [state] and ev.bad == (state == -1) and (state == 1 or not _nonzero(ev)), kw
    two = G.evidence_ref(W, [OPS, OPS], [9, 9], [2, 2], [6, 6], [0, 1], [QUERY, QUERY], [7, 7], 10)
    again = G.evidence_ref(W, [OPS], [9], [2], [6], [1], [QUERY], [7], 10, into=_one(0).evidence)
    assert two.evidence == again.evidence and two.evidence[4][1] == list(_col(20)) and two.evidence[4][2] == list(_col(20))


def test_a_table_of_ones_counts_what_the_pileup_counts_and_strands_mirror():
    """every op string of at most 6 columns: the two walks pick the same columns, and a reverse read is its forward twin"""
    rng = np.random.default_rng(5)
    ones = [[1] * 94 for _ in range(3)]
    checked = 0
    for n in range(1, 7):
        for ops in itertools.product((1, 2, 3, 4), repeat=n):
            n_ref, n_query = sum(v != 4 for v in ops), sum(v != 3 for v in ops)
            if n_ref == 0:
                continue
            query = [int(v) for v in rng.integers(0, 6, size=n_query)]
            qual = [int(v) for v in rng.integers(0, 20, size=n_query)]
            lo, cap = int(rng.integers(0, 3)), int(rng.integers(0, 30))
            R = n_ref + 3
            rev = ([list(ops)], [n], [lo], [n_ref], [1], [query + [0]], [n_query], R)
            fwd = ([list(ops)[::-1]], [n], [lo], [n_ref], [0], [C.revcomp(query) + [0]], [n_query], R)
            for args, q in ((rev, qual + [0]), (fwd, qual[::-1] + [0])):
                pile = P.pileup_ref(*args, qual=[q], min_qual=5)
                ev = G.evidence_ref(ones, *args, qual=[q], min_qual=5, cap=[cap])
                assert ev.used.tolist() == pile.used.tolist() and ev.bad == pile.bad == 0
                assert all(ev.evidence[p][k] == [int(pile.counts[p, 0, k] + pile.counts[p, 1, k])] * 3 for p in range(R) for k in range(5)), ops
            a = G.evidence_ref(W, *rev, qual=[qual + [0]], min_qual=5, cap=[cap])
            b = G.evidence_ref(W, *fwd, qual=[qual[::-1] + [0]], min_qual=5, cap=[cap])
            assert a.evidence == b.evidence, ops
            checked += 1
    assert checked > 5000


def _call(name, **kw):
    row = next(r for r in K.HAND_ROWS if r["name"] == name)
    out = G.call_position(row["E"], row["counts"], row["ins_lengths"], row["ins_bases"], row["r"], K.hand_weights(), K.HAND_GAP_QUAL,
                          kw.get("alt_prior", K.HAND_PRIOR), kw.get("min_depth", K.HAND_MIN_DEPTH))
    return out


def test_genotype_rules_by_hand_at_every_tie():
    assert len({r["name"] for r in K.HAND_ROWS}) == len(K.HAND_ROWS)
    # (G, G) costs 0 + 25, (A, G) 5 + 10 + 10: a tie, and reference/reference wins it against the smaller index
    alleles, gq, qual, flags, *_, costs = _call("homref_ties_het")
    assert (alleles, gq, qual, flags) == ((2, 2), 0, 0, 0) and costs[1] == costs[5] == 25 and sorted(costs)[2] == 45
    alleles, gq, qual, flags, *_, costs = _call("het_wins_by_one")
    assert (alleles, gq, qual, flags) == ((1, 2), 1, 1, G.SUBSTITUTION | G.HET_FLAG) and costs[1] == 24
    # (A, G) and (A, C) both cost 0 + 5 + 20 + 10; reference/reference 50 + 20 + 20
    alleles, gq, qual, flags, *_, costs = _call("two_hets_tie")
    assert (alleles, gq, qual, flags) == ((1, 2), 0, 55, G.SUBSTITUTION | G.HET_FLAG) and costs[1] == costs[2] == 35 and costs[0] == 90
    assert _call("base_and_deletion")[:4] == ((3, 0), 38, 66, G.SUBSTITUTION | G.DELETION | G.HET_FLAG)       # 14, then 52; (A, A) 80
    assert _call("ref_and_deletion")[:4] == ((1, 0), 38, 86, G.DELETION | G.HET_FLAG)                        # 14, then 52; (A, A) 100
    assert _call("deleted_twice")[:4] == ((0, 0), 9, 30, G.DELETION)                                         # 10, 19, and (C, C) 40
    assert _call("depth_2")[:4] == ((1, 1), 0, 0, G.LOW_DEPTH) and _call("depth_3")[:4] == ((2, 2), 9, 30, G.SUBSTITUTION)
    assert _call("depth_3", min_depth=4)[:4] == ((1, 1), 0, 0, G.LOW_DEPTH) and _call("depth_2", min_depth=2)[:4] == ((2, 2), 9, 30, G.SUBSTITUTION)
    for name, r in (("r_0", 0), ("r_7", 7), ("r_negative", 0), ("r_300", 255)):
        alleles, gq, qual, flags, *_, costs = _call(name)
        assert (alleles, gq, qual, flags) == ((r, r), 0, 0, 0) and costs[5] == 0 and costs[1] == 9 and costs[0] == 40, name      # no prior
    assert _call("r_0_shallow")[:4] == ((0, 0), 0, 0, G.LOW_DEPTH)
    assert _call("depth_3")[-1][5] == 10 and _call("depth_3")[-1][0] == 40                                   # with r a base: the prior
    assert _call("gq_at_the_clamp")[:4] == ((1, 1), 2 ** 31 - 1, 0, 0) and _call("gq_past_the_clamp")[:4] == ((1, 1), 2 ** 31 - 1, 0, 0)
    assert _call("gq_at_the_clamp")[-1][1] == 2 ** 31 - 1 and _call("gq_past_the_clamp")[-1][1] == 2 ** 31
    assert _call("qual_at_the_clamp")[:4] == ((1, 1), 2 ** 31 - 1, 2 ** 31 - 1, G.SUBSTITUTION)
    assert _call("qual_past_the_clamp")[:4] == ((1, 1), 2 ** 31 - 1, 2 ** 31 - 1, G.SUBSTITUTION)
    assert _call("qual_at_the_clamp")[-1][5] - 17 == 2 ** 31 - 1 and _call("qual_past_the_clamp")[-1][5] - 17 == 2 ** 31
    assert _call("both_far_past")[:4] == ((1, 1), 2 ** 31 - 1, 2 ** 31 - 1, G.SUBSTITUTION)
    # the insertion, as (copies, labels, gq, qual): 0 copies 10 n + m, one 3 (n + m) + 10, two n + 10 m + 10
    ins = lambda name, **kw: _call(name, **kw)[4:8]                  # noqa: E731
    assert ins("ins_none") == (0, [], 18, 0) and ins("ins_tie_0_and_1") == (0, [], 0, 0)                     # 4, 22, 50; 22, 22, 32
    assert ins("ins_one_copy") == (1, [2, 3], 1, 9) and _call("ins_one_copy")[3] == G.INSERTION | G.INS_HET  # 31, 22, 23
    assert ins("ins_two_copies") == (2, [2, 3], 8, 26) and _call("ins_two_copies")[3] == G.INSERTION         # 40, 22, 14
    assert ins("ins_more_than_depth") == (2, [2, 3], 10, 35)           # n = 5 of d = 4: m = 0; 50, 25, 15; lengths tie: the shorter
    assert ins("ins_empty_sequence") == (0, [], 0, 0) and _call("ins_empty_sequence")[3] == 0
    assert ins("ins_short_of_depth") == (0, [], 0, 0) and _call("ins_short_of_depth")[3] == G.LOW_DEPTH
    assert ins("ins_short_of_depth", min_depth=2) == (2, [2, 3], 4, 8)                                       # n = d = 2: 20, 16, 12
    assert ins("ins_two_copies", alt_prior=36) == (0, [], 0, 0) and ins("ins_two_copies", alt_prior=35) == (2, [2, 3], 1, 1)     # 40, 48, 40: fewer copies
    assert _call("ins_on_a_substituted_site")[:4] == ((1, 2), 1, 1, G.SUBSTITUTION | G.HET_FLAG | G.INSERTION)
    assert _call("ins_beside_r_outside")[:4] == ((0, 0), 0, 0, G.INSERTION) and ins("ins_beside_r_outside") == (2, [2], 8, 26)


def test_records_by_hand():
    """1/2, the `*` allele, a deletion run whose zygosity changes, a run at position 0, an insertion on a substituted site"""
    ref = [1, 2, 3, 4, 1, 2, 3, 4]
    alleles = [(0, 0), (2, 0), (1, 4), (4, 0), (2, 2), (2, 0), (0, 0), (1, 2)]
    flags = [G.DELETION, G.DELETION | G.HET_FLAG, G.SUBSTITUTION | G.HET_FLAG, G.DELETION | G.HET_FLAG, G.SUBSTITUTION | G.INSERTION | G.INS_HET,
             G.DELETION | G.HET_FLAG, G.DELETION, G.SUBSTITUTION | G.HET_FLAG]
    alleles[2], flags[2] = (1, 0), G.SUBSTITUTION | G.DELETION | G.HET_FLAG                                  # A beside the deletion at a C
    R = len(ref)
    counts = np.zeros((R, 2, 6), dtype=np.int64)
    counts[:, 0, 0] = np.arange(R) + 3
    pile = P.Pile(counts, np.zeros((R, 3), dtype=np.int64), np.zeros((R, 2, 4), dtype=np.int64), None, 0)
    ins_bases = np.zeros((R, 2), dtype=np.uint8)
    ins_bases[4] = (4, 1)
    calls = G.Calls(np.array(alleles, dtype=np.uint8), np.arange(R) * 100 + 1, np.arange(R) * 1000 + 2, np.array(flags, dtype=np.uint8),
                    np.array([0, 0, 0, 0, 1, 0, 0, 0], dtype=np.uint8), np.array([0, 0, 0, 0, 2, 0, 0, 0], dtype=np.uint8), ins_bases,
                    np.arange(R) * 10 + 5, np.arange(R) * 10 + 7, None)
    assert G.records_ref(ref, calls, pile) == [
        (0, "del", (1, 2), ((2,),), "1/1", 2, 1, 3),                                                         # at 0: anchored on the next base
        (0, "del", (1, 2, 3, 4), ((1,),), "0/1", 1002, 101, 4),                                              # the zygosity changed at 1
        (2, "sub", (3,), ((1,), ()), "1/2", 2002, 201, 5),
        (4, "sub", (1,), ((2,),), "1/1", 4002, 401, 7),
        (4, "del", (1, 2), ((1,),), "0/1", 5002, 501, 8),
        (4, "ins", (1,), ((1, 4, 1),), "0/1", 47, 45, 7),
        (5, "del", (2, 3), ((2,),), "1/1", 6002, 601, 9),
        (7, "sub", (4,), ((1,), (2,)), "1/2", 7002, 701, 10)]


@pytest.mark.parametrize("noisy", [False, True])
def test_conditions_of_the_planted_diploid_run(noisy):
    run, host = K.diploid(noisy), K.diploid_host(noisy)
    assert len(run["reads"]) == 128 and all(300 <= len(r) <= 500 for r in run["reads"]) and run["strand"] == [b & 1 for b in range(128)]
    assert [r[4] for r in run["records"]] == ["0/1", "1/1"] * 6 and sorted(r[1] for r in run["records"]) == ["del"] * 3 + ["ins"] * 3 + ["sub"] * 6
    wrong = int((run["qual"] == K.Q_WRONG).sum())
    assert (wrong == 0) if not noisy else 0.015 < wrong / int(run["lengths"].sum()) < 0.025
    assert host["pile"].used.tolist() == [1] * 128 and host["evidence"].used.tolist() == [1] * 128
    assert [r[:5] for r in host["records"]] == run["records"]        # the committed seeds' condition
    calls = host["calls"]
    called = {r[0] + (r[1] == "del") + t for r in run["records"] for t in range(len(r[2]) - 1 if r[1] == "del" else 1)}
    for p in range(C.PLANT_REF):
        if p not in called:
            assert calls.alleles[p].tolist() == [run["ref"][p]] * 2 and int(calls.flags[p]) & ~G.LOW_DEPTH == 0, p
    assert int((calls.flags & G.LOW_DEPTH != 0).sum()) == 0 and all(r[5] > 0 and r[6] > 0 for r in host["records"])
