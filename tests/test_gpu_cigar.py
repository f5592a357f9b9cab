"""GPU: cigar_runs / cigar_ops (csrc/wn_cigar.hip through wavenet_speech_amd/sam.py) against the reference of tests/cigar_ref.py.
Everything the kernels write is an integer, so every comparison is exact equality; tests/test_cigar_ref.py holds the reference
itself on the CPU, and the cases are built once in tests/cigar_cases.py.  T = 256 op columns (and 256 runs) is the kernels' tile."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import cigar_cases as K
from tests import cigar_ref as C
from tests import opwalk_cases as O
from tests import pileup_cases as PC
from tests.gpu_calls import alignment as _alignment, capture as _capture, weights as _weights
from tests.gpu_util import DEV, assert_equal_arrays as _equal, dev as _dev, i32 as _i32, strided as _strided
from tests.gpu_util import no_stale_flags  # noqa: F401

pytestmark = pytest.mark.gpu


def _encode_args(t):
    """a Batch as the arguments of cigar_runs"""
    return _alignment(t.ops, t.ops_len), _i32(t.lo), _i32(t.ref_len), _i32(t.strand), _i32(t.query_len), len(t.reference)


def _encode_want(t, eqx=True, max_cigar=None, keep=None):
    """the reference with the limits cigar_runs derives from the row width"""
    M = min(t.ops.shape[1], 8192)
    return C.encode_ref(t.ops, t.ops_len, t.lo, t.ref_len, t.strand, t.query_len, M, len(t.reference), eqx=eqx,
                        max_cigar=min(t.ops.shape[1], 2 * M + 1) + 2 if max_cigar is None else max_cigar, keep=keep)


def _assert_rows(got, want):
    assert got.cigar.dtype == torch.int32 and got.used.dtype == torch.int8 and got.n_cigar.dtype == torch.int32
    _equal(got.used.cpu().numpy(), want.used, "used")
    _equal(got.n_cigar.cpu().numpy(), want.n_cigar, "n_cigar")
    for k, name in enumerate(("pos", "ref_span", "clip_front", "clip_back", "nm")):
        _equal(getattr(got, name).cpu().numpy(), want.fields[:, k], name)
    _equal(got.cigar.cpu().numpy(), want.cigar.view(np.int32), "cigar")          # the zeroes behind n_cigar included


def _assert_ops(got, want):
    a = got.alignment
    assert a.ops.dtype == torch.uint8 and got.used.dtype == torch.int8 and bool(torch.isnan(a.score).all())
    _equal(got.used.cpu().numpy(), want.used, "used")
    _equal(a.ops_len.cpu().numpy(), want.ops_len, "ops_len")
    _equal(got.ref_lengths.cpu().numpy(), want.ref_lengths, "ref_lengths")
    _equal(torch.stack([a.matches, a.mismatches, a.gaps, a.length], 1).cpu().numpy(), want.stats, "stats")
    _equal(a.ops.cpu().numpy(), want.ops, "ops")                                  # the zeroes behind ops_len included


def _flags_report(count, what):
    if count:
        with pytest.raises(RuntimeError, match="wavenet_speech_amd.%s: %d " % (what, count)):
            W.check_device_flags()
    W.check_device_flags()


def _decode(t, strict=False, cigar=None, query=None):
    return W.cigar_ops(_dev(t.cigar) if cigar is None else cigar, _i32(t.n_cigar), _i32(t.pos), _i32(t.strand), _i32(t.reference),
                       _dev(t.query) if query is None else query, _i32(t.query_len), max_ops=t.max_ops, strict=strict)


# ---- the encoder --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eqx", [True, False])
def test_lengths_run_placements_and_degenerate_rows_on_both_strands(eqx):
    t = K.encode_batch()
    want = _encode_want(t, eqx)
    assert want.bad == 0 and sorted(set(want.used.tolist())) == [0, 1]
    got = W.cigar_runs(*_encode_args(t), eqx=eqx)
    _assert_rows(got, want)
    assert got.eqx is eqx and got.strand.cpu().tolist() == t.strand.tolist()
    _flags_report(0, "cigar_runs")
    if eqx:
        b = t.names.index("example/1")
        assert W.cigar_strings(got)[b] == "1S1=2D1=1I1X2=2S" and W.cigar_strings(got)[t.names.index("example/0")] == "2S2=1X1I1=2D1=1S"


def test_strided_rows_and_keep():
    t = K.encode_batch()
    want = _encode_want(t, keep=t.keep)
    assert want.used[4] == 0 and want.used[9] == 0 and want.n_cigar[9] == 0
    ops = _strided(t.ops, False)
    assert not ops.is_contiguous()
    aln = W.PairwiseAlignment(None, None, None, None, None, ops, _i32(t.ops_len))
    got = W.cigar_runs(aln, _i32(t.lo), _i32(t.ref_len), torch.tensor(t.strand.tolist(), device=DEV), t.query_len.tolist(), len(t.reference),
                       keep=torch.tensor(t.keep, device=DEV))
    _assert_rows(got, want)
    # the decoder reads strided runs and strided int64 labels
    runs = K.Runs(t.names, want.cigar.view(np.int32), want.n_cigar, want.fields[:, 0], t.strand, t.query, t.query_len, t.reference, t.ops.shape[1])
    cigar, query = _strided(runs.cigar, False), _strided(t.query.astype(np.int64), False)
    assert not cigar.is_contiguous() and not query.is_contiguous()
    _assert_ops(_decode(runs, cigar=cigar, query=query), C.decode_ref(runs.cigar, runs.n_cigar, runs.pos, runs.strand, t.reference, t.query, t.query_len, runs.max_ops))
    _flags_report(0, "cigar_ops")


def test_a_row_of_exactly_max_cigar_runs_and_one_of_one_more():
    t, max_cigar = K.overflow_batch()
    want = _encode_want(t, max_cigar=max_cigar)
    assert want.used.tolist() == [1, -2, 1, -2] and want.n_cigar.tolist() == [600, 601, 600, 601]
    got = W.cigar_runs(*_encode_args(t), max_cigar=max_cigar)
    _assert_rows(got, want)                                          # the count is reported, the row is zero: never truncated
    _flags_report(2, "cigar_runs")
    with pytest.raises(ValueError, match="wavenet_speech_amd.sam_records: read 'over/0' has no CIGAR"):
        W.sam_records(t.names, t.query, t.query_len, got, "chr")


def test_one_read_at_the_limits():
    """8192 query labels in 65535 + 8192 columns, one deletion run over 256 tiles, on both strands; and back"""
    t = K.limit_read()
    assert t.ops.shape[1] == 65535 + 8192 and t.query_len.tolist() == [8192, 8192] and t.ops_len.tolist() == [65535 + 8192] * 2
    want = _encode_want(t)
    got = W.cigar_runs(*_encode_args(t))
    _assert_rows(got, want)
    back = W.cigar_ops(got.cigar, got.n_cigar, got.pos, got.strand, _i32(t.reference), _dev(t.query), _i32(t.query_len), max_ops=65535 + 8192)
    _assert_ops(back, C.decode_ref(want.cigar.view(np.int32), want.n_cigar, want.fields[:, 0], t.strand, t.reference, t.query, t.query_len, 65535 + 8192))
    _equal(back.alignment.ops.cpu().numpy(), t.ops, "the row itself: it has no end columns")
    _flags_report(0, "cigar_ops")


def test_bad_rows_draw_pileups_verdict():
    """an op of 0 or 5, a length out of range, labels not consumed, strand 2, the skipped kinds (tests/opwalk_cases.py) and a window
    past R: used is pileup's for the same rows, one by one"""
    t = O.batch()
    lo = t.lo.copy()
    past = O.rows_of(O.VALID)[-1]
    lo[past] = O.R - int(t.ref_len[past]) + 1
    b = K.Batch(t.kind, t.ops, t.ops_len, lo, t.ref_len, t.strand, t.query, t.query_len, np.zeros(O.R, dtype=np.int32), None)
    want = _encode_want(b)
    n_bad = len(O.rows_of(O.BAD, O.STRAND_ONLY)) + 1
    assert want.bad == n_bad and want.used[past] == -1 and set(want.used[O.rows_of(O.SKIPPED)].tolist()) == {0}
    got = W.cigar_runs(*_encode_args(b))
    _assert_rows(got, want)
    _flags_report(n_bad, "cigar_runs")
    pile = W.pileup(_alignment(t.ops, t.ops_len), _i32(lo), _i32(t.ref_len), _i32(t.strand), _dev(t.query), _i32(t.query_len), O.R)
    assert torch.equal(got.used, pile.used), (got.used.cpu().tolist(), pile.used.cpu().tolist())
    _flags_report(n_bad, "pileup")


# ---- the decoder --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strict", [False, True])
def test_hand_made_run_tables(strict):
    """H, P and zero-length runs, N, a code of 9, every header kind, sums that would wrap 32 bits, strict on and off"""
    t = K.decode_batch()
    want = C.decode_ref(t.cigar, t.n_cigar, t.pos, t.strand, t.reference, t.query, t.query_len, t.max_ops, strict=strict)
    assert want.used[t.names.index("wrap_columns")] == -1 and want.used[t.names.index("eq_over_mismatch/1")] == (-1 if strict else 1)
    _assert_ops(_decode(t, strict), want)
    _flags_report(want.bad, "cigar_ops")


def test_run_tables_at_the_tile_edges():
    """255, 256, 257 and 1100 runs of one column each: the scan over the runs and the search over its offsets"""
    batch, t = K.run_edge_batch()
    want = C.decode_ref(t.cigar, t.n_cigar, t.pos, t.strand, t.reference, t.query, t.query_len, t.max_ops, strict=True)
    assert want.bad == 0
    _equal(want.ops, batch.ops, "rows without end columns come back as they were")
    _assert_ops(_decode(t, strict=True), want)
    _assert_rows(W.cigar_runs(*_encode_args(batch)), _encode_want(batch))
    _flags_report(0, "cigar_ops")


# ---- the round trips ------------------------------------------------------------------------------------------------------------------

def test_round_trips_and_piles_on_random_rows():
    t = K.random_batch(41)
    R = len(t.reference)
    rows = W.cigar_runs(*_encode_args(t))
    _assert_rows(rows, _encode_want(t))
    query, n_query = _dev(t.query), _i32(t.query_len)
    back = W.cigar_ops(rows.cigar, rows.n_cigar, rows.pos, rows.strand, _i32(t.reference), query, n_query, max_ops=t.ops.shape[1], strict=True)
    fields = torch.stack([rows.pos, rows.ref_span, rows.clip_front, rows.clip_back], 1).cpu().numpy()
    ops, ops_len = back.alignment.ops.cpu().numpy(), back.alignment.ops_len.cpu().numpy()
    for b in range(len(t.names)):                                    # decode(encode(A)): the clips, then the span, in read orientation
        want = K.round_trip_row(K.walk_of(t, b), fields[b])
        assert ops[b, :ops_len[b]].tolist() == (want[::-1] if t.strand[b] else want), t.names[b]
    assert torch.equal(back.lo, rows.pos) and torch.equal(back.ref_lengths, rows.ref_span) and back.used.cpu().tolist() == [1] * len(t.names)
    again = W.cigar_runs(back.alignment, back.lo, back.ref_lengths, rows.strand, n_query, R, max_cigar=int(rows.cigar.shape[1]))
    for name in ("cigar", "n_cigar", "pos", "ref_span", "clip_front", "clip_back", "nm", "used"):      # encode(decode(C)) == C
        assert torch.equal(getattr(again, name), getattr(rows, name)), name
    # end columns enter nothing: the tables of the decoded rows are bitwise the tables of the original rows
    original = (_alignment(t.ops, t.ops_len), _i32(t.lo), _i32(t.ref_len), rows.strand, query, n_query, R)
    decoded = (back.alignment, back.lo, back.ref_lengths, rows.strand, query, n_query, R)
    for a, b in zip(W.pileup(*original), W.pileup(*decoded)):
        assert torch.equal(a, b)
    for a, b in zip(W.pileup_evidence(*original, _weights()), W.pileup_evidence(*decoded, _weights())):
        assert torch.equal(a, b)
    _flags_report(0, "cigar_ops")


def test_one_graph_holds_both_kernels_and_two_runs_are_bitwise_identical():
    t = K.random_batch(43, B=16, n_max=600)
    args = _encode_args(t)
    reference, query, n_query = _i32(t.reference), _dev(t.query), _i32(t.query_len)

    def step():
        rows = W.cigar_runs(*args)
        back = W.cigar_ops(rows.cigar, rows.n_cigar, rows.pos, rows.strand, reference, query, n_query, max_ops=t.ops.shape[1])
        return tuple(rows[:8]) + (back.alignment.ops, back.alignment.ops_len, back.ref_lengths, back.alignment.matches, back.used)

    eager = [x.clone() for x in step()]
    graph, captured = _capture(step)
    for x in captured:
        x.fill_(77)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for a, b, c in zip(eager, captured, step()):
        assert torch.equal(a, b) and torch.equal(a, c)
    _flags_report(0, "cigar_ops")


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

def test_the_planted_run_through_sam_text_and_back():
    """map -> align -> cigar_runs -> sam_records -> parse_sam -> cigar_ops -> pileup -> call_consensus: the calls and the consensus of
    the direct chain, exactly; and the decoded rows go into left_align and quality_profile as they stand"""
    run = PC.planted(True)
    labels, lengths = _dev(run["labels"]), _dev(run["lengths"])
    index = W.read_index(_i32(run["ref"]), k=11, w=5)
    m = W.map_reads(labels, lengths, index)
    lo, _ = m.window(PC.PLANT_FLANK)
    window, window_len = m.labels(PC.PLANT_FLANK)
    aln = W.pairwise_align(window, window_len, labels, lengths)
    pile = W.pileup(aln, lo, window_len, m.strand, labels, lengths, index.R)
    calls = W.call_consensus(pile, index)

    rows = W.cigar_runs(aln, lo, window_len, m.strand, lengths, index.R)
    names = ["read%d" % b for b in range(PC.PLANT_READS)]
    text = W.sam_header("chr", index.R) + W.sam_records(names, labels, lengths, rows, "chr", reference=index, mapq=m.mapq())
    r = W.parse_sam(text)
    assert r.names == names and r.strand.tolist() == run["strand"] and torch.equal(r.labels, labels.cpu()[:, :r.labels.shape[1]])
    c = W.cigar_ops(r.cigar.to(DEV), r.n_cigar, r.pos, r.strand, index, r.labels.to(DEV), r.lengths, max_ops=int(aln.ops.shape[1]), strict=True)
    assert c.used.cpu().tolist() == [1] * PC.PLANT_READS
    pile2 = W.pileup(c.alignment, c.lo, c.ref_lengths, r.strand.to(DEV), r.labels.to(DEV), r.lengths, index.R)
    for a, b in zip(pile, pile2):
        assert torch.equal(a, b)
    calls2 = W.call_consensus(pile2, index)
    for name, a, b in zip(calls._fields, calls, calls2):
        assert torch.equal(a, b), name
    assert calls2.consensus.cpu().tolist() == run["sample"]
    # the windows of the decoded rows in read orientation, cut on the host
    spans = list(zip(c.lo.cpu().tolist(), c.ref_lengths.cpu().tolist(), run["strand"]))
    cut, cut_len = PC.rows([PC.window_labels(run["ref"], p, n, s) for p, n, s in spans])
    settled = W.left_align(c.alignment, _dev(cut), _i32(cut_len), r.labels.to(DEV), r.lengths, r.strand.to(DEV)).settled
    assert int(settled.min()) >= 0
    W.quality_profile(c.alignment, _dev(cut), _i32(cut_len), r.labels.to(DEV), r.lengths)
    _flags_report(0, "cigar_ops")
