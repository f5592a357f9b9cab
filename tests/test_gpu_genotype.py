"""GPU: pileup_evidence / call_genotypes / genotype_records (csrc/wn_genotype.hip through wavenet_speech_amd/genotype.py) against the
reference of tests/genotype_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality, ties
included; tests/test_genotype_ref.py holds the reference itself on the CPU, and the planted diploid runs are built once in
tests/genotype_cases.py.  Every shape is tiny: T = 256 op columns is the evidence kernel's tile, S = 256 positions the call kernel's."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import genotype_cases as K
from tests import genotype_ref as G
from tests import pileup_cases as C
from tests import pileup_ref as P
from tests.gpu_calls import TABLE, alignment as _alignment, assert_evidence as _assert_evidence, assert_genotypes as _assert_calls
from tests.gpu_calls import evidence_both as _both, pile_dev as _pile_dev, weights as _weights
from tests.gpu_util import DEV, dev as _dev, i32 as _i32

pytestmark = pytest.mark.gpu
T, S = 256, 256


def test_tile_edges_on_both_strands():
    rng = np.random.default_rng(1)
    strings = [C.random_ops(rng, n) for n in (T - 1, T, T + 1, 2 * T + 1)]
    strings += [[1] * (T - 6) + [4] * 12 + [1] * 9,                  # an insertion run and a deletion run across the first tile edge
                [2] * (T - 6) + [3] * 12 + [2] * 9,
                [3] * T + [1] * 20 + [4] * 3,                        # the first aligned column on a tile edge, end columns before it
                [4] * (T - 1) + [1] * 20 + [3] * 3,
                [4] * 7 + [1] * (T - 8) + [1] + [3] * 30,            # the last aligned column at T - 1, and at T
                [3] * 7 + [1] * (T - 7) + [1] + [4] * 30,
                [1] * T + [4, 4] + [3] + [4] + [1] * (T - 3)]
    strings += [s[::-1] for s in strings[4:]]                        # a reverse-strand read walks its columns back to front
    reads = [C.read(s, rng) for s in strings]
    ops, n_ref, query, qual = C.cols(reads)
    n = len(reads)
    cap = [int(v) for v in rng.integers(0, 120, size=n)]
    for strands in ([0] * n, [1] * n, [b & 1 for b in range(n)]):
        got, want = _both(ops, [3 * b for b in range(n)], n_ref, strands, query, 3 * n + 2 * T + 60, qual=qual, min_qual=12, cap=cap, gap_qual=17)
        assert want.used.tolist() == [1] * n and sum(want.evidence[p][4][2] for p in range(len(want.evidence))) > 0
    W.check_device_flags()


def test_windows_clamped_at_both_ends_and_a_reference_of_one():
    rng = np.random.default_rng(2)
    reads = [C.read(C.random_ops(rng, 70), rng, odd=0.0) for _ in range(6)] + [C.read([1] * 40, rng, odd=0.0)] * 2
    ops, n_ref, query, qual = C.cols(reads)
    R = max(n_ref)
    lo = [0 if b & 1 else R - r[1] for b, r in enumerate(reads[:6])] + [0, R - 40]          # a window at 0, a window that ends at R
    for strands in ([0] * 8, [1] * 8, [0, 1, 1, 0, 0, 1, 1, 0]):
        got, want = _both(ops, lo, n_ref, strands, query, R, qual=qual)
        assert want.used.tolist() == [1] * 8 and any(any(c) for c in want.evidence[0]) and any(any(c) for c in want.evidence[R - 1])
    got, want = _both([[1], [2], [4, 1, 4], [3]], [0] * 4, [1] * 4, [0, 1, 1, 0], [[3], [3], [1, 4, 1], []], 1, query_len=[1, 1, 3, 0], flat_qual=30)
    col = [TABLE[t][30] for t in range(3)]
    assert want.evidence == [[col, col, col, [0] * 3, [0] * 3]] and want.used.tolist() == [1, 1, 1, 0]
    W.check_device_flags()


def test_quals_caps_and_flat_qual():
    rng = np.random.default_rng(4)
    reads = [C.read([4, 1, 1, 4, 4, 4, 1, 3, 2, 1, 4], rng, odd=0.0) for _ in range(6)]
    ops, n_ref, query, _ = C.cols(reads)
    quals = [[9, 10, 11, 9, 10, 9, 10, 9, 10, 0], [10] * 10, [93] * 10, [0, 93, 0, 93, 0, 93, 0, 93, 0, 93], [0] * 10, [92, 93] * 5]
    args = (ops, [0, 1, 2, 3, 0, 1], n_ref, [0, 1, 0, 1, 1, 0], query, 12)
    for min_qual in (0, 1, 10, 11, 93):                              # quals 0 and 93 on both sides of min_qual
        got, want, pile = _both(*args, qual=quals, min_qual=min_qual, pile=True)
        ones, _ = _both(*args, table=[[1] * 94] * 3, qual=quals, min_qual=min_qual)
        assert torch.equal(ones.evidence[:, :, 0], pile.counts[:, :, :5].sum(1).long())          # the same columns went to `other`
    for cap in ([9] * 6, [10] * 6, [11] * 6, [0] * 6, [93] * 6, [255] * 6, [0, 9, 10, 92, 93, 94]):      # below, at and above q
        got, want = _both(*args, qual=quals, min_qual=10, cap=cap, gap_qual=10)
    capped, _ = _both(*args, qual=quals, cap=[10] * 6, gap_qual=30)
    clipped, _ = _both(*args, qual=[[min(v, 10) for v in q] for q in quals], gap_qual=10)
    assert torch.equal(capped.evidence, clipped.evidence)
    for flat in (0, 20, 93):                                         # no qual: flat_qual on every base, min_qual asks nothing
        got, want = _both(*args, flat_qual=flat, min_qual=50, gap_qual=93 - flat, cap=[255, 93, 20, 19, 0, 21])
    got, want = _both(*args, flat_qual=41)
    same, _ = _both(*args, qual=[[41] * 10] * 6)
    assert torch.equal(got.evidence, same.evidence)
    W.check_device_flags()


def test_skipped_reads_are_not_looked_at():
    rng = np.random.default_rng(5)
    good = C.read([3, 1, 2, 4, 1, 3, 1, 4], rng, odd=0.0)
    ops = [good[0], good[0], good[0], [3] * 6, [3, 3, 3, 4, 4], good[0], [9] * 8]
    query = [good[2], good[2], good[2], [], [1, 2], good[2], good[2]]
    # unmapped (strand -1, with a window that would be bad), ref_lengths 0, keep false, empty, end columns only, good, unmapped garbage
    got, want = _both(ops, [0, 0, 0, 0, 0, 1, -7], [6, 0, 6, 6, 3, 6, 99], [-1, 0, 1, 0, 1, 1, -2], query, 8,
                      keep=[True, True, False, True, True, True, True], ops_len=[8, 8, 8, 6, 5, 8, 200], query_len=[6, 6, 6, 0, 2, 6, -3])
    assert want.used.tolist() == [0, 0, 0, 0, 0, 1, 0] and want.bad == 0 and sum(1 for p in want.evidence for c in p if any(c)) == 5
    W.check_device_flags()                                           # nothing is reported


def test_bad_pairs_add_nothing_and_are_counted():
    rng = np.random.default_rng(6)
    ops, n_ref, query, _ = C.read([3, 1, 2, 4, 4, 1, 3, 1, 4], rng, odd=0.0)
    n_query = len(query)
    bad = [dict(ops=ops[:4] + [0] + ops[5:]), dict(ops=ops[:4] + [5] + ops[5:]), dict(ops=ops[:4] + [255] + ops[5:]), dict(ops_len=13),
           dict(ops_len=-1), dict(ops_len=8), dict(ops=ops[:-1] + [3]), dict(n_ref=n_ref + 1), dict(n_ref=n_ref - 1), dict(n_ref=-2),
           dict(query_len=n_query - 1), dict(query_len=n_query + 1), dict(query_len=n_query + 4), dict(query_len=-1), dict(strand=2),
           dict(strand=7), dict(lo=-1), dict(lo=20 - n_ref + 1), dict(lo=2 ** 31 - 3), dict(qual=[94] + [5] * (n_query - 1)),
           dict(qual=[5] * (n_query - 1) + [255])]
    rows = [dict(ops=ops, ops_len=len(ops), n_ref=n_ref, query_len=n_query, strand=b & 1, lo=b % 3, qual=[5] * n_query) for b in range(len(bad) + 4)]
    for b, change in enumerate(bad):
        rows[b + 2].update(change)                                   # good reads before, between and after
    only_good, _ = _both([ops] * 4, [0, 1, (len(bad) + 2) % 3, (len(bad) + 3) % 3], [n_ref] * 4, [0, 1, len(bad) & 1, (len(bad) + 1) & 1], [query] * 4, 20,
                         qual=[[5] * n_query] * 4)
    W.check_device_flags()
    got, want = _both([r["ops"] + [1] * (12 - len(r["ops"])) for r in rows], [r["lo"] for r in rows], [r["n_ref"] for r in rows],
                      [r["strand"] for r in rows], [query + [1, 1] for _ in rows], 20, qual=[r["qual"] + [99, 99] for r in rows],
                      ops_len=[r["ops_len"] for r in rows], query_len=[r["query_len"] for r in rows])
    assert want.bad == len(bad) and want.used.tolist() == [1, 1] + [-1] * len(bad) + [1, 1]
    assert torch.equal(got.evidence, only_good.evidence)             # the good reads' sums are intact
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.pileup_evidence: %d pair\\(s\\) whose ops do not fit" % len(bad)):
        W.check_device_flags()
    W.check_device_flags()                                           # raised once


def test_the_carry_of_a_true_64_bit_add():
    """a cell preset to 2^32 - 1 and one preset to 2^51, each taking one add of weight 1 and one of 2^20"""
    table = [[0] * 94 for _ in range(3)]
    table[0][3], table[0][7], table[1][3], table[1][7], table[2][3], table[2][7] = 1, 2 ** 20, 2 ** 20, 1, 1, 1
    preset = [[[0] * 3 for _ in range(5)] for _ in range(4)]
    preset[1][0] = [2 ** 32 - 1, 2 ** 32 - 1, 2 ** 51]               # the reads show A at position 1 and T at position 2
    preset[2][3] = [2 ** 51, 2 ** 32 - 2 ** 20, 2 ** 32 - 2]
    into = (W.Evidence(torch.tensor(preset, dtype=torch.int64, device=DEV), None), G.Evidence(preset, None, 0))
    got, want = _both([[1, 1]] * 2, [1, 1], [2, 2], [0, 0], [[1, 4]] * 2, 4, table=table, qual=[[3, 7], [7, 3]], into=into)
    assert want.evidence[1][0] == [2 ** 32 + 2 ** 20, 2 ** 32 + 2 ** 20, 2 ** 51 + 2] and want.evidence[2][3] == [2 ** 51 + 2 ** 20 + 1, 2 ** 32 + 1, 2 ** 32]
    assert got.evidence is into[0].evidence and got.evidence[1, 0].tolist() == want.evidence[1][0]
    W.check_device_flags()


def test_contention_on_one_locus():
    rng = np.random.default_rng(8)
    ops, n_ref, query, qual = C.read([1] * 12 + [4, 4] + [1] * 10 + [3] + [2] * 17, rng, odd=0.05)
    assert n_ref == 40
    got, want = _both([ops] * 300, [0] * 300, [40] * 300, [0] * 300, [query] * 300, 40, qual=[qual] * 300, gap_qual=2)
    assert want.evidence[22][4] == [300 * TABLE[t][2] for t in range(3)]
    reads = [r for r in (C.read(C.random_ops(rng, 42), rng) for _ in range(300)) if r[1] <= 40]
    ops, n_ref, query, qual = C.cols(reads)
    n = len(reads)
    got, want = _both(ops, [40 - r[1] if b % 3 else 0 for b, r in enumerate(reads)], n_ref, [int(v) for v in rng.integers(0, 2, size=n)], query, 40,
                      qual=qual, cap=[int(v) for v in rng.integers(0, 94, size=n)])
    assert n > 200
    W.check_device_flags()


def test_accumulation_over_batches_reproducibility_and_the_pileup_counts():
    rng = np.random.default_rng(9)
    reads = [C.read(C.random_ops(rng, int(rng.integers(40, 300))), rng) for _ in range(24)]
    args = lambda part, first=0: (C.cols(part)[0], [2 * b for b in range(first, first + len(part))], C.cols(part)[1],      # noqa: E731
                                  [b & 1 for b in range(first, first + len(part))], C.cols(part)[2], 400)
    kw = lambda part: dict(qual=C.cols(part)[3], min_qual=9)          # noqa: E731
    whole, _ = _both(*args(reads), **kw(reads))
    again, _ = _both(*args(reads), **kw(reads))
    assert torch.equal(whole.evidence, again.evidence) and torch.equal(whole.used, again.used)   # bitwise: integer addition commutes
    first = _both(*args(reads[:12]), **kw(reads[:12]))
    second = _both(*args(reads[12:], 12), into=first, **kw(reads[12:]))
    assert second[0].evidence is first[0].evidence and torch.equal(second[0].evidence, whole.evidence)      # accumulated in place
    # a table of ones: every cell is pileup's count of the same batch over both strands
    ones, _, pile = _both(*args(reads), table=[[1] * 94] * 3, pile=True, **kw(reads))
    assert torch.equal(ones.evidence, pile.counts[:, :, :5].sum(1).long()[:, :, None].expand(400, 5, 3)) and torch.equal(ones.used, pile.used)
    with pytest.raises(ValueError, match="wavenet_speech_amd.pileup_evidence: into.evidence must be a contiguous int64 tensor of shape \\(300, 5, 3\\)"):
        W.pileup_evidence(_alignment(*C.rows([reads[0][0]], dtype=np.uint8)), _i32([0]), _i32([reads[0][1]]), _i32([0]), _i32([reads[0][2]]),
                          _i32([len(reads[0][2])]), 300, _weights(), into=whole)
    W.check_device_flags()


def test_strided_rows_and_int64_labels():
    rng = np.random.default_rng(10)
    reads = [C.read(C.random_ops(rng, 90), rng) for _ in range(5)]
    ops_rows, ops_len = C.rows(C.cols(reads)[0], dtype=np.uint8)
    q_rows, q_len = C.rows(C.cols(reads)[2])
    qual_rows = C.rows(C.cols(reads)[3], width=q_rows.shape[1], dtype=np.uint8)[0]
    lo, n_ref, strand = [0, 3, 6, 9, 12], C.cols(reads)[1], [0, 1, 0, 1, 1]
    want = G.evidence_ref(TABLE, ops_rows, ops_len, lo, n_ref, strand, q_rows, q_len, 120, qual=qual_rows, min_qual=12)
    wide = lambda a, fill: _dev(np.concatenate([a, np.full((a.shape[0], 37), fill, dtype=a.dtype)], axis=1))    # noqa: E731
    ops_wide, q_wide, qual_wide = wide(ops_rows, 7), wide(q_rows.astype(np.int64), 2), wide(qual_rows, 200)
    aln = W.PairwiseAlignment(None, None, None, None, None, ops_wide[:, :ops_rows.shape[1]], _i32(ops_len))
    args = (aln, _i32(lo), _i32(n_ref), torch.tensor(strand, device=DEV), q_wide[:, :q_rows.shape[1]], torch.tensor(q_len.tolist(), device=DEV), 120,
            _weights())
    got = W.pileup_evidence(*args, qual=qual_wide[:, :q_rows.shape[1] + 5], min_qual=12)
    _assert_evidence(got, want)
    W.check_device_flags()


# ---- call_genotypes -------------------------------------------------------------------------------------------------------------

def _calls_both(pile, evidence, ref, table=TABLE, **kw):
    """pile: a pileup_ref Pile of numpy tables; evidence: nested lists [R][5][3] -> (Genotypes, reference Calls), equal exactly"""
    want = G.call_genotypes_ref(pile, evidence, ref, table, **kw)
    got = W.call_genotypes(_pile_dev(pile), W.Evidence(torch.tensor(evidence, dtype=torch.int64, device=DEV), None), _dev(np.asarray(ref, dtype=np.int64)),
                           _weights(table), return_costs=True, **kw)
    _assert_calls(got, want)
    return got, want


@pytest.mark.parametrize("R", [1, S - 1, S, S + 1])
def test_call_genotypes_at_the_tile_edges(R):
    rng = np.random.default_rng(R)
    ref = rng.integers(0, 6, size=R)
    for max_ins, min_depth, prior, gap_qual in ((2, 3, 3000, 20), (0, 1, 0, 0), (8, 6, 7, 93), (3, 4, 2 ** 30, 5)):
        pile = C.random_pile(rng, R, max_ins)
        evidence = (rng.integers(0, 40, size=(R, 5, 3)) * (rng.random((R, 5, 1)) < 0.6)).tolist()      # small: ties are common
        got, want = _calls_both(pile, evidence, ref, min_depth=min_depth, alt_prior=prior, gap_qual=gap_qual)
        assert tuple(got.costs.shape) == (R, 15) and tuple(got.ins_bases.shape) == (R, max_ins)
    plain = W.call_genotypes(_pile_dev(pile), W.Evidence(torch.tensor(evidence, device=DEV), None), _dev(ref), _weights())
    assert plain.costs is None and tuple(plain.alleles.shape) == (R, 2)


def _hand_pile(rows):
    return P.Pile(np.array([r["counts"] for r in rows], dtype=np.int64), np.array([r["ins_lengths"] for r in rows], dtype=np.int64),
                  np.array([r["ins_bases"] for r in rows], dtype=np.int64), None, 0)


def test_genotype_rules_by_hand():
    """the rows of tests/test_genotype_ref.py::test_genotype_rules_by_hand_at_every_tie as one table"""
    rows = K.HAND_ROWS
    pile, evidence, ref = _hand_pile(rows), [r["E"] for r in rows], [r["r"] for r in rows]
    for min_depth, prior in ((K.HAND_MIN_DEPTH, K.HAND_PRIOR), (2, K.HAND_PRIOR), (4, K.HAND_PRIOR), (3, 36), (3, 35), (3, 0)):
        got, want = _calls_both(pile, evidence, ref, table=K.hand_weights(), gap_qual=K.HAND_GAP_QUAL, alt_prior=prior, min_depth=min_depth)
    got, want = _calls_both(pile, evidence, ref, table=K.hand_weights(), gap_qual=K.HAND_GAP_QUAL, alt_prior=K.HAND_PRIOR, min_depth=K.HAND_MIN_DEPTH)
    at = {r["name"]: p for p, r in enumerate(rows)}
    assert got.alleles[at["homref_ties_het"]].tolist() == [2, 2] and got.alleles[at["het_wins_by_one"]].tolist() == [1, 2]
    assert got.gq[at["gq_at_the_clamp"]].item() == got.gq[at["gq_past_the_clamp"]].item() == 2 ** 31 - 1
    assert got.flags[at["ins_one_copy"]].item() == W.Genotypes.INSERTION | W.Genotypes.INS_HET and got.ins_copies[at["ins_tie_0_and_1"]].item() == 0


def test_counts_and_costs_beside_their_limits():
    top = 2 ** 31 - 1
    counts = np.zeros((6, 2, 6), dtype=np.int64)
    counts[0, 0, 0], counts[1, 0, 0], counts[1, 1, 3] = top, top - 1, 1                          # d = 2^31 - 1 twice, as one cell and as two
    counts[2, 0, 1] = top - 1                                                                    # d = 2^31 - 2
    counts[3, :, :5] = top                                                                       # d = 10 (2^31 - 1): a 64-bit sum
    counts[4, 0, 2], counts[5, 0, 2] = 5, 5
    ins_lengths = np.zeros((6, 9), dtype=np.int64)
    ins_lengths[3], ins_lengths[4, 0], ins_lengths[5, 8] = top, top, top                         # n = 9 (2^31 - 1) times 2^20: past 2^54
    ins_bases = np.zeros((6, 8, 4), dtype=np.int64)
    ins_bases[3:, :, 2] = top
    pile = P.Pile(counts, ins_lengths, ins_bases, None, 0)
    big = 2 ** 51
    evidence = [[[big - 1, big - 2, big - 3]] * 5, [[big, 1, big]] * 5, [[0, 0, 0]] * 5, [[big - 1] * 3, [big] * 3, [1, big, 2], [big, 2, big - 5], [3, 3, 3]],
                [[2 ** 31, 2 ** 31 - 1, 2 ** 32]] * 5, [[0, big, 0], [big, 0, big], [0, 0, 0], [big, big, big], [1, 1, 1]]]
    table = [[2 ** 20] * 94, [2 ** 20 - 1] * 94, [2 ** 20] * 94]
    for min_depth in (top, top - 1, 1):
        for prior in (2 ** 30, 0):
            got, want = _calls_both(pile, evidence, [1, 2, 3, 4, 1, 0], table=table, min_depth=min_depth, alt_prior=prior, gap_qual=93)
    got, want = _calls_both(pile, evidence, [1, 2, 3, 4, 1, 0], table=table, min_depth=top, alt_prior=2 ** 30, gap_qual=93)
    flags = want.flags.tolist()
    assert flags[0] == 0 and flags[1] & G.HET_FLAG and flags[2] == G.LOW_DEPTH and flags[3] & G.INSERTION      # both sides of d = min_depth = 2^31 - 1
    assert max(max(c) for c in want.costs) > 2 ** 53 and int(want.ins_gq.max()) == top


# ---- the closed loop on the planted diploid runs ----------------------------------------------------------------------------------

@pytest.mark.parametrize("noisy", [False, True])
def test_closed_loop_on_the_planted_diploid_runs(noisy):
    run = K.diploid(noisy)
    labels, lengths, qual = _dev(run["labels"]), _dev(run["lengths"]), _dev(run["qual"])
    index = W.read_index(_i32(run["ref"]), k=11, w=5)
    m = W.map_reads(labels, lengths, index)
    lo, length = m.window(C.PLANT_FLANK)
    ref_rows, ref_len = m.labels(C.PLANT_FLANK)
    assert torch.equal(length, ref_len) and m.strand.cpu().tolist() == run["strand"]
    aln = W.pairwise_align(ref_rows, ref_len, labels, lengths)
    aln = W.left_align(aln, ref_rows, ref_len, labels, lengths, m.strand).alignment
    w = W.genotype_weights(K.SCALE)
    assert w.table.tolist() == K.weights()
    pile = W.pileup(aln, lo, ref_len, m.strand, labels, lengths, index.R, qual=qual, min_qual=K.MIN_QUAL)
    ev = W.pileup_evidence(aln, lo, ref_len, m.strand, labels, lengths, index.R, w, qual=qual, min_qual=K.MIN_QUAL)
    host = (aln.ops.cpu().numpy(), aln.ops_len.cpu().numpy(), lo.cpu().tolist(), ref_len.cpu().tolist(), m.strand.cpu().tolist(), run["labels"],
            run["lengths"], index.R)
    want_pile = P.pileup_ref(*host, qual=run["qual"], min_qual=K.MIN_QUAL)
    want_ev = G.evidence_ref(K.weights(), *host, qual=run["qual"], min_qual=K.MIN_QUAL)
    _assert_evidence(ev, want_ev)                                    # the reference fed with the GPU's own windows and ops
    assert want_ev.used.tolist() == [1] * K.READS and torch.equal(ev.used, pile.used)
    assert np.array_equal(pile.counts.cpu().numpy(), want_pile.counts)
    calls = W.call_genotypes(pile, ev, index, w)                     # alt_prior None: 30 * scale
    want_calls = G.call_genotypes_ref(want_pile, want_ev.evidence, run["ref"], K.weights(), alt_prior=K.ALT_PRIOR)
    _assert_calls(calls, want_calls)
    records = W.genotype_records(index, calls, pile)
    assert [tuple(v) for v in records] == G.records_ref(run["ref"], want_calls, want_pile)
    assert [tuple(v)[:5] for v in records] == run["records"]         # the planted records with the planted GT
    lines = W.vcf_genotype_records("chr", index, calls, pile, w)
    assert len(lines) == 12 and [l.split("\t")[9].split(":")[0] for l in lines] == ["0/1", "1/1"] * 6
    assert all(l.endswith("\n") and int(l.split("\t")[5]) > 0 and l.split("\t")[8] == "GT:GQ" for l in lines)
    W.check_device_flags()
