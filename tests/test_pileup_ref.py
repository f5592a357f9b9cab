"""CPU: the host reference of the pileup and the consensus calls (tests/pileup_ref.py) against hand-worked piles, strand symmetry
over every short op string, the calling rules at every tie and on both sides of min_depth and num / den, and the two planted runs
of tests/pileup_cases.py, whose seeds are chosen so that the host chain alone returns the sample genome and the planted edits."""
import itertools

import numpy as np

from tests import pileup_cases as C
from tests import pileup_ref as P

OPS = [3, 1, 2, 4, 4, 1, 3, 1, 4]             # end, A, G, insertion of 2, G, deletion, other, end
QUERY = [1, 2, 3, 4, 2, 0, 1]


def _one(strand, ops=OPS, query=QUERY, lo=2, n_ref=6, R=10, **kw):
    if kw.get("qual") is not None:
        kw = dict(kw, qual=[kw["qual"]])
    return P.pileup_ref([ops], [len(ops)], [lo], [n_ref], [strand], [query], [len(query)], R, **kw)


def _nonzero(t):
    return {tuple(int(v) for v in k): int(t[tuple(k)]) for k in np.argwhere(t)}


def test_hand_worked_forward_pile():
    pile = _one(0)
    assert pile.used.tolist() == [1] and pile.bad == 0
    assert _nonzero(pile.counts) == {(3, 0, 0): 1, (4, 0, 1): 1, (5, 0, 1): 1, (6, 0, P.DEL): 1, (7, 0, P.OTHER): 1}
    assert _nonzero(pile.ins_lengths) == {(4, 1): 1}
    assert _nonzero(pile.ins_bases) == {(4, 0, 2): 1, (4, 1, 3): 1}


def test_hand_worked_reverse_pile():
    """reference index i of the ops is forward position 7 - i; the labels are complemented and the insertion is turned round"""
    pile = _one(1)
    assert _nonzero(pile.counts) == {(6, 1, 3): 1, (5, 1, 2): 1, (4, 1, 2): 1, (3, 1, P.DEL): 1, (2, 1, P.OTHER): 1}
    assert _nonzero(pile.ins_lengths) == {(4, 1): 1}
    assert _nonzero(pile.ins_bases) == {(4, 0, 0): 1, (4, 1, 1): 1}


def test_hand_worked_limits_and_states():
    assert _nonzero(_one(0, max_ins=1).ins_lengths) == {(4, 1): 1} and _nonzero(_one(0, max_ins=1).ins_bases) == {(4, 0, 2): 1}
    assert _nonzero(_one(0, max_ins=0).ins_lengths) == {(4, 0): 1} and _one(0, max_ins=0).ins_bases.shape == (10, 0, 4)
    qual = [20, 9, 10, 9, 10, 10, 0]
    pile = _one(0, qual=qual, min_qual=10)
    assert _nonzero(pile.counts) == {(3, 0, 0): 1, (4, 0, P.OTHER): 1, (5, 0, 1): 1, (6, 0, P.DEL): 1, (7, 0, P.OTHER): 1}
    assert _nonzero(pile.ins_bases) == {(4, 0, 2): 1} and _nonzero(pile.ins_lengths) == {(4, 1): 1}
    assert _nonzero(_one(0, qual=qual, min_qual=0).counts) == _nonzero(_one(0).counts)
    for kw, state in ((dict(strand=-1), 0), (dict(n_ref=0), 0), (dict(keep=[False]), 0), (dict(ops=[3] * 6 + [4] * 7), 0),
                      (dict(strand=2), -1), (dict(lo=-1), -1), (dict(lo=5), -1), (dict(ops=OPS[:-1] + [5]), -1), (dict(ops=OPS[:-1] + [0]), -1),
                      (dict(ops=OPS[:-1]), -1), (dict(ops=OPS + [3]), -1), (dict(qual=[94] + [0] * 6), -1), (dict(qual=[93] * 7), 1),
                      (dict(lo=4), 1), (dict(lo=0), 1)):
        args = dict(dict(strand=0), **kw)
        pile = _one(args.pop("strand"), **args)
        assert pile.used.tolist() == [state] and pile.bad == (state == -1), kw
        if state != 1:
            assert not pile.counts.any() and not pile.ins_lengths.any() and not pile.ins_bases.any()
    two = P.pileup_ref([OPS, OPS], [9, 9], [2, 2], [6, 6], [0, 1], [QUERY, QUERY], [7, 7], 10)
    again = P.pileup_ref([OPS], [9], [2], [6], [1], [QUERY], [7], 10, into=_one(0))
    assert all(np.array_equal(a, b) for a, b in zip(two[:3], again[:3]))
    assert two.counts[:, :, :5].sum() == 8


def test_strand_symmetry_over_every_short_op_string():
    rng = np.random.default_rng(5)
    checked = 0
    for n in range(1, 7):
        for ops in itertools.product((1, 2, 3, 4), repeat=n):
            n_ref, n_query = sum(v != 4 for v in ops), sum(v != 3 for v in ops)
            if n_ref == 0:
                continue
            query = [int(v) for v in rng.integers(0, 6, size=n_query)]
            qual = [int(v) for v in rng.integers(0, 20, size=n_query)]
            lo = int(rng.integers(0, 3))
            a = P.pileup_ref([list(ops)], [n], [lo], [n_ref], [1], [query + [0]], [n_query], n_ref + 3, qual=[qual + [0]], min_qual=5, max_ins=2)
            b = P.pileup_ref([list(ops)[::-1]], [n], [lo], [n_ref], [0], [C.revcomp(query) + [0]], [n_query], n_ref + 3, qual=[qual[::-1] + [0]],
                             min_qual=5, max_ins=2)
            assert a.used.tolist() == b.used.tolist() and a.bad == b.bad == 0
            assert np.array_equal(a.counts[:, 1], b.counts[:, 0]) and not a.counts[:, 0].any() and not b.counts[:, 1].any(), ops
            assert np.array_equal(a.ins_lengths, b.ins_lengths) and np.array_equal(a.ins_bases, b.ins_bases), ops
            checked += 1
    assert checked > 5000


def _call(counts_fwd, counts_rev=(0,) * 6, r=1, ins_lengths=(0, 0, 0), ins_bases=((0,) * 4,) * 2, min_depth=3, num=1, den=2):
    return P.call_position([list(counts_fwd), list(counts_rev)], list(ins_lengths), [list(s) for s in ins_bases], r, min_depth, num, den)


def test_calling_rules_at_ties_and_thresholds():
    # min_depth on both sides; `other` is no depth
    assert _call((0, 2, 0, 0, 0, 9), r=1) == (1, [], P.LOW_DEPTH, (0, 0))
    assert _call((0, 2, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), r=1) == (2, [], P.SUBSTITUTION, (2, 1))
    assert _call((0, 2, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), r=2) == (2, [], 0, (2, 1))
    # count * den > num * d on both sides: 2 of 4 is not more than half, 3 of 5 is
    assert _call((0, 2, 1, 1, 0, 0), r=1) == (1, [], P.AMBIGUOUS, (0, 0))
    assert _call((0, 3, 1, 1, 0, 0), r=1) == (2, [], P.SUBSTITUTION, (3, 0))
    assert _call((0, 3, 1, 1, 0, 0), r=1, num=3, den=5) == (1, [], P.AMBIGUOUS, (0, 0))
    assert _call((0, 3, 1, 0, 0, 0), r=1, num=3, den=5) == (2, [], P.SUBSTITUTION, (3, 0))
    assert _call((1, 1, 1, 1, 0, 0), r=3, num=0, den=1) == (3, [], 0, (1, 0))                   # a four-way tie goes to the reference
    assert _call((1, 1, 1, 1, 0, 0), r=0, num=0, den=1) == (1, [], P.SUBSTITUTION, (1, 0))      # then to the smaller label
    assert _call((0, 0, 2, 2, 2, 0), r=4, num=0, den=1) == (4, [], 0, (2, 0))
    assert _call((0, 0, 2, 2, 2, 0), r=1, num=0, den=1) == (3, [], P.SUBSTITUTION, (2, 0))
    assert _call((0, 0, 0, 2, 2, 0), r=1, num=0, den=1) == (4, [], P.SUBSTITUTION, (2, 0))      # deletion last
    assert _call((0, 0, 0, 1, 3, 0), r=4) == (0, [], P.DELETION, (3, 0))
    assert _call((0, 0, 0, 0, 2, 0), (0, 0, 0, 0, 2, 0), r=7) == (0, [], P.DELETION, (2, 2))
    assert _call((4, 0, 0, 0, 0, 0), r=7) == (1, [], P.SUBSTITUTION, (4, 0))
    assert _call((1, 1, 0, 0, 0, 0), r=300, min_depth=1) == (255, [], P.AMBIGUOUS, (0, 0))      # labels are kept as bytes
    assert _call((0,) * 6, r=-4, min_depth=1) == (0, [], P.LOW_DEPTH, (0, 0))
    # insertions: n * den > num * d on both sides, min_depth, the fullest length with ties to the shorter, the last column as max_ins
    full = ((0, 5, 0, 0), (0, 0, 2, 2))
    assert _call((4, 0, 0, 0, 0, 0), ins_lengths=(0, 2, 0), ins_bases=full) == (1, [], 0, (4, 0))
    assert _call((4, 0, 0, 0, 0, 0), ins_lengths=(0, 3, 0), ins_bases=full) == (1, [2, 3], P.INSERTION, (4, 0))
    assert _call((2, 0, 0, 0, 0, 0), ins_lengths=(0, 3, 0), ins_bases=full) == (1, [], P.LOW_DEPTH, (2, 0))
    assert _call((4, 0, 0, 0, 0, 0), ins_lengths=(2, 2, 0), ins_bases=full) == (1, [2], P.INSERTION, (4, 0))
    assert _call((4, 0, 0, 0, 0, 0), ins_lengths=(1, 1, 2), ins_bases=full) == (1, [2, 3], P.INSERTION, (4, 0))
    assert _call((4, 0, 0, 0, 0, 0), ins_lengths=(0, 3, 0), ins_bases=((0, 0, 0, 0), (0, 0, 2, 2))) == (1, [], 0, (4, 0))
    assert _call((4, 0, 0, 0, 0, 0), ins_lengths=(0, 3, 0), ins_bases=((0, 0, 0, 1), (0, 0, 0, 0))) == (1, [4], P.INSERTION, (4, 0))
    assert _call((0, 0, 0, 0, 4, 0), ins_lengths=(3, 0, 0), ins_bases=full) == (0, [2], P.DELETION | P.INSERTION, (4, 0))
    assert P.call_position([[4, 0, 0, 0, 0, 0], [0] * 6], [9], np.zeros((0, 4)), 1, 3, 1, 2) == (1, [], 0, (4, 0))      # max_ins = 0


def test_emit_and_records_by_hand():
    ref = [1, 2, 3, 4, 1, 2]
    counts = np.zeros((6, 2, 6), dtype=np.int64)
    for p, k in enumerate((P.DEL, P.DEL, 2, 0, P.DEL, 1)):           # deleted, deleted, kept C, T -> A, deleted, kept G
        counts[p, p & 1, k] = 4
    ins_lengths, ins_bases = np.zeros((6, 3), dtype=np.int64), np.zeros((6, 2, 4), dtype=np.int64)
    ins_lengths[2, 1], ins_bases[2, 0, 3], ins_bases[2, 1, 0] = 3, 3, 3
    pile = P.Pile(counts, ins_lengths, ins_bases, None, 0)
    calls = P.call_consensus_ref(pile, ref)
    assert calls.call.tolist() == [0, 0, 3, 1, 0, 2] and calls.ins_len.tolist() == [0, 0, 2, 0, 0, 0]
    assert calls.consensus.tolist() == [3, 4, 1, 1, 2] and calls.offsets.tolist() == [0, 0, 0, 3, 4, 4, 5]
    assert P.variants_ref(ref, calls, pile) == [(0, "del", (1, 2, 3), (3,), 4, 4, 4, 0), (2, "ins", (3,), (3, 4, 1), 4, 3, None, None),
                                                (3, "sub", (4,), (1,), 4, 4, 0, 4), (3, "del", (4, 1), (4,), 4, 4, 4, 0)]
    gone = P.call_consensus_ref(P.Pile(np.tile(np.array([0, 0, 0, 0, 3, 0]), (4, 2, 1)), np.zeros((4, 1), dtype=np.int64),
                                       np.zeros((4, 0, 4), dtype=np.int64), None, 0), [1, 2, 3, 4])
    assert gone.consensus.tolist() == [] and gone.offsets.tolist() == [0] * 5 and gone.flags.tolist() == [P.DELETION] * 4
    pile4 = P.Pile(np.tile(np.array([0, 0, 0, 0, 3, 0]), (4, 2, 1)), np.zeros((4, 1), dtype=np.int64), np.zeros((4, 0, 4), dtype=np.int64), None, 0)
    assert P.variants_ref([1, 2, 3, 4], gone, pile4) == [(0, "del", (1, 2, 3, 4), (), 6, 6, 3, 3)]


def _planted_run(noisy):
    run, host = C.planted(noisy), C.planted_host(noisy)
    assert host["pile"].bad == 0 and host["pile"].used.tolist() == [1] * C.PLANT_READS
    depth = host["pile"].counts[:, :, :5].sum((1, 2))
    assert depth[run["records"][0][0]:run["records"][-1][0] + 1].min() >= 3          # no position between the edits is LOW_DEPTH
    assert [int(v) for v in host["calls"].consensus] == run["sample"]
    assert [v[:4] for v in host["variants"]] == run["records"]
    assert len(run["records"]) == 12 and sorted(len(r[2]) - len(r[3]) for r in run["records"]) == [-4, -2, -1] + [0] * 6 + [1, 2, 3]


def test_planted_run_without_noise_gives_the_sample_and_the_edits():
    _planted_run(False)


def test_planted_run_with_noise_gives_the_sample_and_the_edits():
    run, clean = C.planted(True), C.planted(False)
    differing = sum(a != b for x, y in zip(run["reads"], clean["reads"]) for a, b in zip(x, y))
    total = sum(len(x) for x in run["reads"])
    assert 0.01 * total < differing < 0.03 * total and [len(x) for x in run["reads"]] == [len(x) for x in clean["reads"]]
    _planted_run(True)
