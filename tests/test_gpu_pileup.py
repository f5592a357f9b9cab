"""GPU: pileup / call_consensus / variant_records (csrc/wn_pileup.hip through wavenet_speech_amd/pileup.py) against the reference
of tests/pileup_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality, ties included;
tests/test_pileup_ref.py holds the reference itself on the CPU, and the planted runs are built once in tests/pileup_cases.py.
Every shape is tiny: T = 256 op columns is the pileup kernel's tile, S = 256 positions the tile of the call and emit kernels."""
import functools

import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import pileup_cases as C
from tests import pileup_ref as P
from tests.gpu_calls import U, alignment as _alignment, assert_consensus as _assert_calls, assert_pile as _assert_pile, pile_both as _both
from tests.gpu_calls import pile_dev as _to_device
from tests.gpu_util import DEV, dev as _dev, i32 as _i32

pytestmark = pytest.mark.gpu
T, S = U.TILE, U.SCAN_TILE
_read = functools.partial(C.read, quals=False)      # pileup takes no qualities: none are drawn
CALLED = P.SUBSTITUTION | P.DELETION | P.INSERTION


def test_tile_edges_on_both_strands():
    rng = np.random.default_rng(1)
    strings = [C.random_ops(rng, n) for n in (T - 1, T, T + 1, 2 * T + 1)]
    strings += [[1] * (T - 6) + [4] * 12 + [1] * 9,                  # an insertion run and a deletion run across the first tile edge
                [2] * (T - 6) + [3] * 12 + [2] * 9,
                [1] * 5 + [4] * (T + 40) + [1] * 5,                  # an insertion longer than a tile
                [3] * T + [1] * 20 + [4] * 3,                        # the first aligned column on a tile edge, end columns before it
                [4] * (T - 1) + [1] * 20 + [3] * 3,
                [4] * 7 + [1] * (T - 8) + [1] + [3] * 30,            # the last aligned column at T - 1, and at T
                [3] * 7 + [1] * (T - 7) + [1] + [4] * 30,
                [1] * (T - 1) + [4] + [1] * T + [4] + [1],           # one-column runs that end a tile
                [1] * T + [4, 4] + [3] + [4] + [1] * (T - 3)]        # a run that starts a tile, and runs a deletion apart
    strings += [s[::-1] for s in strings[4:]]                        # a reverse-strand read walks its columns back to front
    reads = [_read(s, rng) for s in strings]
    for strand in (0, 1):
        n = len(reads)
        got, want = _both([r[0] for r in reads], [3 * b for b in range(n)], [r[1] for r in reads], [strand] * n, [r[2] for r in reads],
                          3 * n + 2 * T + 60, max_ins=4)
        assert want.used.tolist() == [1] * n and want.ins_lengths[:, 4].sum() >= 2 and want.counts[:, 1 - strand].sum() == 0
    mixed, _ = _both([r[0] for r in reads], [0] * len(reads), [r[1] for r in reads], [b & 1 for b in range(len(reads))], [r[2] for r in reads],
                     2 * T + 60)
    W.check_device_flags()


def test_windows_clamped_at_both_ends_and_a_reference_of_one():
    rng = np.random.default_rng(2)
    reads = [_read(C.random_ops(rng, 70), rng, odd=0.0) for _ in range(6)] + [_read([1] * 40, rng, odd=0.0)] * 2
    R = max(r[1] for r in reads)
    lo = [0 if b & 1 else R - r[1] for b, r in enumerate(reads[:6])] + [0, R - 40]          # a window at 0, a window that ends at R
    for strands in ([0] * 8, [1] * 8, [0, 1, 1, 0, 0, 1, 1, 0]):
        got, want = _both([r[0] for r in reads], lo, [r[1] for r in reads], strands, [r[2] for r in reads], R)
        assert want.used.tolist() == [1] * 8 and want.counts[0].sum() > 0 and want.counts[R - 1].sum() > 0
    # a reverse read of aligned columns only: its LAST column is position 0
    got, want = _both([[1] * 40], [0], [40], [1], [reads[6][2]], 40)
    assert want.counts[0, 1, 4 - reads[6][2][39]] == 1 and want.counts[39, 1, 4 - reads[6][2][0]] == 1
    got, want = _both([[1], [2], [4, 1, 4], [3]], [0] * 4, [1] * 4, [0, 1, 1, 0], [[3], [3], [1, 4, 1], []], 1, query_len=[1, 1, 3, 0])
    assert want.counts[0].tolist() == [[0, 0, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0]] and want.used.tolist() == [1, 1, 1, 0]
    W.check_device_flags()


@pytest.mark.parametrize("max_ins", [0, 1, 3, 8])
def test_insertion_length_limits(max_ins):
    rng = np.random.default_rng(3)
    strings = [[1] * 4 + [4] * n + [2] * 4 for n in sorted({1, max(max_ins - 1, 1), max(max_ins, 1), max_ins + 1, max_ins + 2, 20})]
    reads = [_read(s, rng, odd=0.0) for s in strings]
    reads.append((reads[-2][0], reads[-2][1], reads[-2][2][:5] + [0] + reads[-2][2][6:]))      # a non-ACGT label inside an insertion
    reads.append((reads[1][0], reads[1][1], reads[1][2][:4] + [7] + reads[1][2][5:]))
    n = len(reads)
    for strands in ([0] * n, [1] * n, [b & 1 for b in range(n)]):
        got, want = _both([r[0] for r in reads], [2] * n, [8] * n, strands, [r[2] for r in reads], 12, max_ins=max_ins)
        assert tuple(got.ins_bases.shape) == (12, max_ins, 4) and want.ins_lengths.sum() == n and want.ins_lengths[:, max_ins].sum() >= 2
        assert got.max_ins == max_ins and got.R == 12 and got.depth.cpu().tolist() == want.counts[:, :, :5].sum((1, 2)).tolist()
    W.check_device_flags()


def test_qual_and_min_qual():
    rng = np.random.default_rng(4)
    reads = [_read([4, 1, 1, 4, 4, 4, 1, 3, 2, 1, 4], rng, odd=0.0) for _ in range(4)]
    quals = [[9, 10, 11, 9, 10, 9, 10, 9, 10, 0], [10] * 10, [93] * 10, [0, 93, 0, 93, 0, 93, 0, 93, 0, 93]]
    args = ([r[0] for r in reads], [0, 1, 2, 3], [r[1] for r in reads], [0, 1, 0, 1], [r[2] for r in reads], 12)
    got10, want10 = _both(*args, qual=quals, min_qual=10)
    assert want10.counts[:, :, P.OTHER].sum() > 0 and want10.ins_bases.sum() < 3 * 4
    got0, want0 = _both(*args, qual=quals, min_qual=0)
    plain, _ = _both(*args)
    assert torch.equal(got0.counts, plain.counts) and torch.equal(got0.ins_bases, plain.ins_bases) and want0.counts[:, :, P.OTHER].sum() == 0
    got93, want93 = _both(*args, qual=quals, min_qual=93)
    assert want93.counts[:, :, :4].sum() > 0
    _both(*args, qual=quals, min_qual=11)
    W.check_device_flags()


def test_skipped_reads_are_not_looked_at():
    rng = np.random.default_rng(5)
    good = _read([3, 1, 2, 4, 1, 3, 1, 4], rng, odd=0.0)
    ops = [good[0], good[0], good[0], [3] * 6, [3, 3, 3, 4, 4], good[0], [9] * 8]
    query = [good[2], good[2], good[2], [], [1, 2], good[2], good[2]]
    # unmapped (strand -1, with a window that would be bad), ref_lengths 0, keep false, empty, end columns only, good, unmapped garbage
    got, want = _both(ops, [0, 0, 0, 0, 0, 1, -7], [6, 0, 6, 6, 3, 6, 99], [-1, 0, 1, 0, 1, 1, -2], query, 8,
                      keep=[True, True, False, True, True, True, True], ops_len=[8, 8, 8, 6, 5, 8, 200], query_len=[6, 6, 6, 0, 2, 6, -3])
    assert want.used.tolist() == [0, 0, 0, 0, 0, 1, 0] and want.bad == 0 and want.counts.sum() == 5
    W.check_device_flags()                                           # nothing is reported


def test_bad_pairs_add_nothing_and_are_counted():
    rng = np.random.default_rng(6)
    ops, n_ref, query = _read([3, 1, 2, 4, 4, 1, 3, 1, 4], rng, odd=0.0)
    n_query = len(query)
    bad = [dict(ops=ops[:4] + [0] + ops[5:]), dict(ops=ops[:4] + [5] + ops[5:]), dict(ops=ops[:4] + [255] + ops[5:]), dict(ops_len=13),
           dict(ops_len=-1), dict(ops_len=8), dict(ops=ops[:-1] + [3]), dict(n_ref=n_ref + 1), dict(n_ref=n_ref - 1), dict(n_ref=-2),
           dict(query_len=n_query - 1), dict(query_len=n_query + 1), dict(query_len=n_query + 4), dict(query_len=-1), dict(strand=2),
           dict(strand=7), dict(lo=-1), dict(lo=20 - n_ref + 1), dict(lo=2 ** 31 - 3), dict(qual=[94] + [5] * (n_query - 1)),
           dict(qual=[5] * (n_query - 1) + [255])]
    rows = [dict(ops=ops, ops_len=len(ops), n_ref=n_ref, query_len=n_query, strand=b & 1, lo=b % 3, qual=[5] * n_query) for b in range(len(bad) + 4)]
    for b, change in enumerate(bad):
        rows[b + 2].update(change)                                   # good reads before, between and after
    only_good, _ = _both([ops] * 4, [0, 1, (len(bad) + 2) % 3, (len(bad) + 3) % 3], [n_ref] * 4, [0, 1, len(bad) & 1, (len(bad) + 1) & 1], [query] * 4, 20)
    W.check_device_flags()
    got, want = _both([r["ops"] + [1] * (12 - len(r["ops"])) for r in rows], [r["lo"] for r in rows], [r["n_ref"] for r in rows],
                      [r["strand"] for r in rows], [query + [1, 1] for _ in rows], 20, qual=[r["qual"] + [99, 99] for r in rows],
                      ops_len=[r["ops_len"] for r in rows], query_len=[r["query_len"] for r in rows])
    assert want.bad == len(bad) and want.used.tolist() == [1, 1] + [-1] * len(bad) + [1, 1]
    assert torch.equal(got.counts, only_good.counts) and torch.equal(got.ins_bases, only_good.ins_bases)     # the good reads' counts are intact
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.pileup: %d pair\\(s\\) whose ops do not fit" % len(bad)):
        W.check_device_flags()
    W.check_device_flags()                                           # raised once


def test_pairs_poisoned_by_pairwise_align_are_bad_pairs():
    rng = np.random.default_rng(7)
    ref = [int(v) for v in rng.integers(1, 5, size=30)]
    ref_rows, query = _i32([ref] * 3), _i32([ref[2:28]] * 3)
    ref_len, query_len = _i32([30, 31, 30]), _i32([26, 26, -1])      # pair 1: a reference length past its row; pair 2: a negative length
    W.check_device_flags()
    aln = W.pairwise_align(ref_rows, ref_len, query, query_len)
    with pytest.raises(RuntimeError, match="pairwise_align"):
        W.check_device_flags()
    assert aln.ops_len.cpu().tolist()[1:] == [0, 0]
    lo, strand = _i32([5, 5, 5]), _i32([0, 0, 0])
    got = W.pileup(aln, lo, ref_len, strand, query, query_len, 40)
    want = P.pileup_ref(aln.ops.cpu().numpy(), aln.ops_len.cpu().numpy(), [5] * 3, [30, 31, 30], [0] * 3, query.cpu().numpy(), [26, 26, -1], 40)
    _assert_pile(got, want)
    assert want.used.tolist() == [1, -1, -1] and want.counts[:, 0, :4].sum() == 26
    with pytest.raises(RuntimeError, match="wavenet_speech_amd.pileup: 2 pair"):
        W.check_device_flags()


def test_contention_on_one_locus():
    rng = np.random.default_rng(8)
    ops, n_ref, query = _read([1] * 12 + [4, 4] + [1] * 10 + [3] + [2] * 17, rng, odd=0.05)
    assert n_ref == 40
    got, want = _both([ops] * 300, [0] * 300, [40] * 300, [0] * 300, [query] * 300, 40)
    assert want.counts.max() == 300 and want.ins_lengths[11, 1] == 300
    reads = [_read(C.random_ops(rng, 42), rng) for _ in range(300)]
    reads = [r for r in reads if r[1] <= 40]
    n = len(reads)
    got, want = _both([r[0] for r in reads], [40 - r[1] if b % 3 else 0 for b, r in enumerate(reads)], [r[1] for r in reads],
                      [int(v) for v in rng.integers(0, 2, size=n)], [r[2] for r in reads], 40)
    assert n > 200 and want.counts[:, 0].sum() > 1000 and want.counts[:, 1].sum() > 1000
    W.check_device_flags()


def test_accumulation_over_batches_and_reproducibility():
    rng = np.random.default_rng(9)
    reads = [_read(C.random_ops(rng, int(rng.integers(40, 300))), rng) for _ in range(24)]
    args = lambda part: ([r[0] for r in part], [2 * b for b in range(len(part))], [r[1] for r in part], [b & 1 for b in range(len(part))],      # noqa: E731
                         [r[2] for r in part], 400)
    whole, _ = _both(*args(reads))
    again, _ = _both(*args(reads))
    for name in ("counts", "ins_lengths", "ins_bases", "used"):
        assert torch.equal(getattr(whole, name), getattr(again, name)), name                     # bitwise: integer addition commutes
    first = _both(*args(reads[:12]))
    a = args(reads[12:])
    second = _both(a[0], [2 * b for b in range(12, 24)], a[2], a[3], a[4], 400, into=first)
    assert second[0].counts is first[0].counts                                                   # accumulated in place
    for name in ("counts", "ins_lengths", "ins_bases"):
        assert torch.equal(getattr(second[0], name), getattr(whole, name)), name
    with pytest.raises(ValueError, match="wavenet_speech_amd.pileup: into.ins_lengths must be a contiguous int32 tensor of shape \\(400, 3\\)"):
        W.pileup(_alignment(*C.rows([reads[0][0]], dtype=np.uint8)), _i32([0]), _i32([reads[0][1]]), _i32([0]), _i32([reads[0][2]]),
                 _i32([len(reads[0][2])]), 400, max_ins=2, into=whole)
    W.check_device_flags()


def test_strided_rows_and_int64_labels():
    rng = np.random.default_rng(10)
    reads = [_read(C.random_ops(rng, 90), rng) for _ in range(5)]
    ops_rows, ops_len = C.rows([r[0] for r in reads], dtype=np.uint8)
    q_rows, q_len = C.rows([r[2] for r in reads])
    qual_rows = rng.integers(0, 40, size=q_rows.shape).astype(np.uint8)
    lo, n_ref, strand = [0, 3, 6, 9, 12], [r[1] for r in reads], [0, 1, 0, 1, 1]
    want = P.pileup_ref(ops_rows, ops_len, lo, n_ref, strand, q_rows, q_len, 120, qual=qual_rows, min_qual=12)
    wide = lambda a, fill: _dev(np.concatenate([a, np.full((a.shape[0], 37), fill, dtype=a.dtype)], axis=1))    # noqa: E731
    ops_wide, q_wide, qual_wide = wide(ops_rows, 7), wide(q_rows.astype(np.int64), 2), wide(qual_rows, 200)
    aln = W.PairwiseAlignment(None, None, None, None, None, ops_wide[:, :ops_rows.shape[1]], _i32(ops_len))
    assert not aln.ops.is_contiguous()
    got = W.pileup(aln, _i32(lo), _i32(n_ref), torch.tensor(strand, device=DEV), q_wide[:, :q_rows.shape[1]], torch.tensor(q_len.tolist(), device=DEV),
                   120, qual=qual_wide[:, :q_rows.shape[1] + 5], min_qual=12)
    _assert_pile(got, want)
    W.check_device_flags()


# ---- call_consensus -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, S - 1, S, S + 1, 3 * S + 2])
def test_call_consensus_at_the_scan_tile_edges(R):
    rng = np.random.default_rng(R)
    ref = rng.integers(0, 6, size=R)
    for max_ins, min_depth, frac in ((2, 3, (1, 2)), (0, 1, (0, 1)), (8, 6, (2, 3)), (3, 4, (1, 1)), (1, 2, (1, 3))):
        pile = C.random_pile(rng, R, max_ins)
        want = P.call_consensus_ref(pile, ref, min_depth, *frac)
        got = W.call_consensus(_to_device(pile), _dev(ref), min_depth=min_depth, min_fraction=frac)
        _assert_calls(got, want)
        assert int(got.offsets[R]) == got.consensus.shape[0] == len(want.consensus)


def test_call_consensus_rules_by_hand():
    """the rows of tests/test_pileup_ref.py::test_calling_rules_at_ties_and_thresholds, as one pile: min_depth 3, more than half"""
    z, full = (0,) * 6, ((0, 5, 0, 0), (0, 0, 2, 2))
    rows = [((0, 2, 0, 0, 0, 9), z, 1), ((0, 2, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), 1), ((0, 2, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), 2),
            ((0, 2, 1, 1, 0, 0), z, 1), ((0, 3, 1, 1, 0, 0), z, 1), ((1, 1, 1, 1, 0, 0), (2, 2, 2, 2, 0, 0), 3), ((3, 3, 3, 3, 0, 0), z, 0),
            ((0, 0, 0, 1, 3, 0), z, 4), ((0, 0, 0, 0, 2, 0), (0, 0, 0, 0, 2, 0), 7), ((4, 0, 0, 0, 0, 0), z, 7), ((1, 1, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), 300),
            (z, z, -4), ((0, 0, 3, 0, 3, 0), z, 3), ((0, 0, 3, 0, 3, 0), z, 1)]
    ins = [((0, 0, 0), ((0,) * 4,) * 2)] * len(rows)
    for lengths, bases in (((0, 2, 0), full), ((0, 3, 0), full), ((2, 2, 0), full), ((1, 1, 2), full), ((0, 3, 0), ((0, 0, 0, 0), (0, 0, 2, 2))),
                           ((0, 3, 0), ((0, 0, 0, 1), (0, 0, 0, 0))), ((0, 0, 3), ((1, 1, 1, 1), (0, 2, 0, 2)))):
        rows.append(((4, 0, 0, 0, 0, 0), z, 1))
        ins.append((lengths, bases))
    rows += [((2, 0, 0, 0, 0, 0), z, 1), ((0, 0, 0, 0, 4, 0), z, 2)]
    ins += [((0, 3, 0), full), ((3, 0, 0), full)]
    pile = P.Pile(np.array([[r[0], r[1]] for r in rows], dtype=np.int64), np.array([i[0] for i in ins], dtype=np.int64),
                  np.array([i[1] for i in ins], dtype=np.int64), None, 0)
    ref = np.array([r[2] for r in rows], dtype=np.int64)
    for min_depth, frac in ((3, (1, 2)), (4, (1, 2)), (3, (3, 5)), (3, (0, 1)), (1, (1, 1))):
        want = P.call_consensus_ref(pile, ref, min_depth, *frac)
        _assert_calls(W.call_consensus(_to_device(pile), _dev(ref), min_depth=min_depth, min_fraction=frac), want)
    want = P.call_consensus_ref(pile, ref, 3, 1, 2)
    assert want.flags[:5].tolist() == [P.LOW_DEPTH, P.SUBSTITUTION, 0, P.AMBIGUOUS, P.SUBSTITUTION]
    assert want.ins_bases[len(rows) - 9:len(rows) - 2].tolist() == [[0, 0], [2, 3], [2, 0], [2, 3], [0, 0], [4, 0], [1, 2]]


def test_a_reference_deleted_whole_gives_an_empty_consensus():
    R = S + 3
    pile = P.Pile(np.tile(np.array([0, 0, 0, 0, 3, 0]), (R, 2, 1)).astype(np.int64), np.zeros((R, 3), dtype=np.int64), np.zeros((R, 2, 4), dtype=np.int64),
                  None, 0)
    ref = np.arange(R) % 4 + 1
    got = W.call_consensus(_to_device(pile), _dev(ref))
    _assert_calls(got, P.call_consensus_ref(pile, ref))
    assert tuple(got.consensus.shape) == (0,) and got.offsets.cpu().tolist() == [0] * (R + 1) and got.flags.cpu().tolist() == [P.DELETION] * R
    lines = W.vcf_records("c", _dev(ref), got, _to_device(pile))
    assert len(lines) == 1 and lines[0].split("\t")[4] == "<DEL>" and len(lines[0].split("\t")[3]) == R


# ---- the closed loop on the planted runs ----------------------------------------------------------------------------------------

def _chain(index, labels, lengths):
    m = W.map_reads(labels, lengths, index)
    lo, length = m.window(C.PLANT_FLANK)
    ref_rows, ref_len = m.labels(C.PLANT_FLANK)
    assert torch.equal(length, ref_len)
    aln = W.pairwise_align(ref_rows, ref_len, labels, lengths)
    pile = W.pileup(aln, lo, ref_len, m.strand, labels, lengths, index.R)
    want = P.pileup_ref(aln.ops.cpu().numpy(), aln.ops_len.cpu().numpy(), lo.cpu().tolist(), ref_len.cpu().tolist(), m.strand.cpu().tolist(),
                        labels.cpu().numpy(), lengths.cpu().tolist(), index.R)
    _assert_pile(pile, want)                                         # the reference fed with the GPU's own windows and ops
    return m, pile, want


@pytest.mark.parametrize("noisy", [False, True])
def test_closed_loop_on_the_planted_runs(noisy):
    run = C.planted(noisy)
    labels, lengths = _dev(run["labels"]), _dev(run["lengths"])
    index = W.read_index(_i32(run["ref"]), k=11, w=5)
    m, pile, want = _chain(index, labels, lengths)
    assert m.strand.cpu().tolist() == run["strand"] and want.used.tolist() == [1] * C.PLANT_READS
    calls = W.call_consensus(pile, index)
    want_calls = P.call_consensus_ref(want, run["ref"])
    _assert_calls(calls, want_calls)
    assert calls.consensus.cpu().tolist() == run["sample"]           # the committed seeds' condition (tests/pileup_cases.py)
    records = W.variant_records(index, calls, pile)
    assert [tuple(v) for v in records] == P.variants_ref(run["ref"], want_calls, want)
    assert [tuple(v)[:4] for v in records] == run["records"]
    lines = W.vcf_records("chr", index, calls, pile)
    assert len(lines) == 12 and all(l.endswith("\n") and l.split("\t")[6] == "PASS" for l in lines)
    assert [int(l.split("\t")[1]) for l in lines] == [r[0] + 1 for r in run["records"]]
    # the consensus goes back in as it stands; the same reads against it show nothing to call
    index2 = W.read_index(calls.consensus, k=11, w=5)
    assert index2.R == len(run["sample"])
    _, pile2, want2 = _chain(index2, labels, lengths)
    calls2 = W.call_consensus(pile2, index2)
    _assert_calls(calls2, P.call_consensus_ref(want2, run["sample"]))
    assert int((calls2.flags & CALLED != 0).sum()) == 0 and torch.equal(calls2.consensus, calls.consensus)
    W.check_device_flags()
