"""CPU: the reference of the realignment against the called haplotypes (tests/realign_ref.py) held to hand-worked rows of every rule,
to the read-end family, and to the conditions of the planted phased run of tests/phase_cases.py in both variants.  No GPU and no
library: plain loops against values worked by hand."""
import numpy as np
import pytest

from tests import pairwise_align_ref as A
from tests import phase_cases as PC
from tests import phase_ref as H
from tests import realign_cases as RC
from tests import realign_ref as RR

# haplotype 0 of tests/realign_cases.py window_calls() over the whole reference, worked by hand: position 0 with its insertion, the
# substitution, two deleted positions, the no-base label, position 6 with max_ins inserted labels, then five kept positions
HAP0 = ([1, 3, 4, 3, 7, 3, 1, 1, 7, 4, 1, 2, 3, 4], [1, 4, 2, 1, 3, 3, 1, 1, 4, 4, 4, 1, 1, 1, 1, 1])
HAP0_REVERSE = ([1, 2, 3, 4, 1, 7, 4, 4, 2, 7, 2, 1, 2, 4], [1, 1, 1, 1, 1, 4, 4, 4, 1, 1, 3, 3, 1, 2, 4, 1])      # 7 stays 7
HAP1 = ([1, 2, 3, 4, 1, 2, 3, 4, 2, 3, 4], [1, 1, 1, 1, 1, 2, 1, 1, 3, 1, 1, 1])


def _rows(w, h, b):
    return [int(v) for v in w.labels[h][b][:w.lengths[h][b]]], [int(v) for v in w.ops[h][b][:w.ops_len[h][b]]]


def test_windows_by_hand():
    hc = RC.window_calls()
    w = RR.haplotype_windows_ref(hc, RC.WINDOW_REF, [0, 0, 0, 6, 6, 3], [12, 12, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1], 16)
    assert w.used.tolist() == [1] * 6 and w.bad == 0
    assert _rows(w, 0, 0) == HAP0 and _rows(w, 0, 1) == HAP0_REVERSE and _rows(w, 1, 0) == HAP1
    assert _rows(w, 0, 2) == ([1], [1])                              # the insertion after the LAST window position is left out
    assert _rows(w, 0, 3) == ([2], [1])                              # ... on the reverse strand too, ins_len == max_ins there
    assert _rows(w, 0, 4) == ([3, 1, 1, 7, 4], [1, 4, 4, 4, 1])      # ins_len == max_ins, inside the window
    assert _rows(w, 0, 5) == ([], [3, 3]) and _rows(w, 1, 5) == ([4, 1], [1, 1])      # an all-deleted window, reverse
    assert not w.labels[0][5].any() and not w.ops[0][2][1:].any()    # zero behind the lengths
    for h in range(2):                                               # the two rows spell the window and the haplotype
        for b, (lo, n, s) in enumerate(zip([0, 0, 0, 6, 6, 3], [12, 12, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1])):
            labels, ops = _rows(w, h, b)
            assert sum(v != 4 for v in ops) == n and sum(v != 3 for v in ops) == len(labels)


def test_windows_skipped_and_bad_and_capacity():
    hc = RC.window_calls()
    lo, n, strand = [0, 0, 0, -1, 5, 0, 0, 0], [12, 0, 12, 3, 8, -2, 12, 12], [-1, 1, 2, 0, 0, 0, 0, 1]
    w = RR.haplotype_windows_ref(hc, RC.WINDOW_REF, lo, n, strand, 16)
    assert w.used.tolist() == [0, 0, -1, -1, -1, -1, 1, 1] and w.bad == 4 and w.lengths[:, :6].sum() == 0 and w.ops_len[:, :6].sum() == 0
    at = RR.haplotype_windows_ref(hc, RC.WINDOW_REF, [0, 6], [12, 2], [0, 0], 16)
    below = RR.haplotype_windows_ref(hc, RC.WINDOW_REF, [0, 6], [12, 2], [0, 0], 15)      # haplotype 0 needs 16: bad on both haplotypes
    assert at.used.tolist() == [1, 1] and below.used.tolist() == [-1, 1] and below.bad == 1 and below.lengths[:, 0].tolist() == [0, 0]
    assert _rows(below, 1, 1) == _rows(at, 1, 1)
    over = RR.HapCalls(hc.call, hc.ins_len, hc.ins_bases[:, :, :2])  # max_ins 2 beside an ins_len of 3
    w = RR.haplotype_windows_ref(over, RC.WINDOW_REF, [0, 6, 7], [6, 1, 5], [0, 0, 0], 16)
    assert w.used.tolist() == [1, -1, 1]                             # checked at every position of the window, the last included


@pytest.mark.parametrize("row", RC.LIFT_ROWS, ids=[r[0] for r in RC.LIFT_ROWS])
def test_composition_by_hand(row):
    _, a, hh, ref, read, want = row
    got = RR.lift_row(a, hh, ref, read, sum(v != 3 for v in hh))
    assert got == want
    assert A.replay(ref, read, got) == ([v for v in ref], [v for v in read])      # consumes both exactly, 1 / 2 by the labels


@pytest.mark.parametrize("row", RC.LIFT_BAD, ids=[r[0] for r in RC.LIFT_BAD])
def test_rows_that_do_not_compose(row):
    _, a, hh, ref, read = row
    assert RR.lift_row(a, hh, ref, read, sum(v != 3 for v in hh)) is None


def test_lift_batch_stats_scores_picks_and_bad_rows():
    pairs = [r[1:5] for r in RC.LIFT_ROWS] + [r[1:] for r in RC.LIFT_BAD]
    n_good, n_bad = len(RC.LIFT_ROWS), len(RC.LIFT_BAD)
    pick = [b & 1 for b in range(len(pairs))]
    args = RC.pair_batch(pairs, pick, H=2)
    out = RR.lift_ref(*args, max_ops=8)
    assert out.bad == n_bad and out.ops_len.tolist()[n_good:] == [0] * n_bad and out.matches.tolist()[n_good:] == [-1] * n_bad
    assert out.score.tolist()[n_good:] == [RR.POISON] * n_bad
    for b, r in enumerate(RC.LIFT_ROWS):
        assert out.ops[b][:out.ops_len[b]].tolist() == r[5] and not out.ops[b][out.ops_len[b]:].any()
        assert out.score[b] == A.rescore(r[5], *A.EMBOSS, True) and out.length[b] == len(r[5])
        assert out.matches[b] + out.mismatches[b] + out.gaps[b] == out.length[b]
    assert out.score[4] == 10 + 10 - 21 - 21 and out.score[5] == 10 - 20 and out.score[8] == 0     # inner runs cost, end runs are free
    wrong = RR.lift_ref(*args[:3], [1 - p for p in pick], *args[4:], max_ops=8)      # the other haplotype's rows hold garbage
    assert wrong.bad == len(pairs)
    short = RR.lift_ref(*args, max_ops=5)                            # "3s before 4s" needs 6
    assert short.bad == n_bad + 1 and short.ops_len[4] == 0 and short.ops_len[9] == 5
    skipped = args[2]._replace(used=np.array([0, -1] + [1] * (len(pairs) - 2), dtype=np.int8))
    out = RR.lift_ref(*args[:2], skipped, *args[3:], max_ops=8)
    assert out.bad == n_bad + 1 and out.score[0] == 0 and out.matches[0] == 0 and out.score[1] == RR.POISON
    for p in (-1, 2):
        assert RR.lift_ref(*args[:3], [p] + pick[1:], *args[4:], max_ops=8).bad == n_bad + 1


def test_random_pairs_replay():
    rng = np.random.default_rng(3)
    for n in (1, 5, 40, 300):
        for _ in range(20):
            a, hh, ref, read = RC.random_pair(rng, n)
            got = RR.lift_row(a, hh, ref, read, sum(v != 3 for v in hh))
            assert got is not None and A.replay(ref, read, got) == (ref, read)
            assert len(got) == len(ref) + len(read) - sum(v <= 2 for v in got)


def test_picks():
    assert RR.picks([[5, 5], [5, 6], [7, 6], [5, 6], [3]], [1, 1, 1, 0, 1]) == ([0, 1, 0, 1, 0], [0, 2, 1, 0, 0], [0, 1, 1, 1, 0])


def test_haplotype_calls_by_hand():
    ref, calls, _ = PC.hand_calls()
    sites = H.sites_ref(calls.flags, calls.alleles)
    assert sites.pos == [1, 2, 3, 5, 7] and PC.HAND_CHAIN.parity == [1, 1, 0, 0, 0]
    hc = RR.haplotype_calls_ref(calls, sites, PC.HAND_CHAIN)
    # alleles (0,0) (2,0) (1,0) (4,0) (2,2) (2,0) (0,0) (1,2): haplotype 0 takes alleles[parity], haplotype 1 the other
    assert hc.call.tolist() == [[0, 0, 0, 4, 2, 2, 0, 1], [0, 2, 1, 0, 2, 0, 0, 2]]
    assert not hc.ins_len.any() and not hc.ins_bases.any()           # the one insertion is INS_HET: on neither haplotype
    both = calls._replace(ins_copies=np.array([0, 0, 0, 0, 2, 0, 0, 0]))
    hc = RR.haplotype_calls_ref(both, sites, PC.HAND_CHAIN)
    assert hc.ins_len.tolist() == [[0, 0, 0, 0, 2, 0, 0, 0]] * 2 and hc.ins_bases[:, 4].tolist() == [[4, 1]] * 2
    none = RR.haplotype_calls_ref(calls, H.Sites([], [], [-1] * 8), H.Chain([], [], [], [], [], [], []))
    assert none.call.tolist() == [[0, 2, 1, 4, 2, 2, 0, 1]] * 2      # S == 0: both haplotypes carry alleles[., 0]


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("edit", RC.END_EDITS, ids=["del1", "del2", "ins2"])
def test_a_read_that_ends_just_past_an_indel(edit, strand):
    """a read of the haplotype that carries the edit, ending 0..6 bases past it: alone against the reference it prefers a mismatch or
    a free end gap at 1 base past a deletion; realigned it shows the edit from 1 base past on"""
    kind, n, inserted = edit
    for past in range(7):
        c = RC.end_case(kind, n, inserted, past, strand)
        own = A.align(c["window"], c["read"]).ops
        r = RR.realign_ref([c["window"]], [c["length"]], [c["read"]], [c["lo"]], [strand], c["hcalls"], RC.END_REF)
        assert r.lifted.bad == 0 and r.windows.bad == 0
        lifted = r.lifted.ops[0][:r.lifted.ops_len[0]].tolist()
        assert A.replay(c["window"], c["read"], lifted) == (c["window"], c["read"])
        before, after = RC.end_support(c, own, kind, n, strand), RC.end_support(c, lifted, kind, n, strand)
        assert after == (1 if past >= 1 else 0) and before <= after
        if kind == "del":
            assert before == (1 if past >= 2 else 0)                 # one base past: a mismatch or nothing
            assert r.hp == [1 if past >= 1 else 0] and (r.delta[0] >= 18) == (past >= 1)      # nothing past the gap: both haplotypes spell the read
        else:
            assert r.hp == [1] and r.delta[0] >= 36                  # the inserted bases themselves decide


@pytest.mark.parametrize("noisy", [False, True])
def test_the_planted_run_meets_its_conditions(noisy):
    run, host, got = PC.planted(noisy), PC.planted_host(noisy), RC.planted_realigned(noisy)
    r = got["realigned"]
    assert r.lifted.bad == 0 and r.windows.bad == 0 and r.windows.used.tolist() == [1] * PC.READS
    _, _, refs = RC.windows_of(run)
    for b in range(PC.READS):                                        # every lifted row against window and read
        row = r.lifted.ops[b][:r.lifted.ops_len[b]].tolist()
        assert A.replay(refs[b], run["reads"][b], row) == (refs[b], run["reads"][b])
        assert r.lifted.score[b] == A.rescore(row, *A.EMBOSS, True)
    own = [A.rescore(host["ops"][b][:host["ops_len"][b]], *A.EMBOSS, True) for b in range(PC.READS)]
    RC.check_conditions(run, host, r, got["before"], got["after"], noisy, own_scores=own)
    # the pick is the planted haplotype: haplotype h of a set carries alleles[s][parity[s] ^ h]
    for b in range(PC.READS):
        if r.hp[b]:
            lo, n = run["window"][b]
            s = next(s for s, p in enumerate(host["sites"].pos) if lo <= p < lo + n)
            truth = run["sites"][host["sites"].pos[s]][(b >> 1) & 1]
            assert host["sites"].alleles[s][host["chain"].parity[s] ^ r.pick[b]] == truth
