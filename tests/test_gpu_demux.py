"""GPU: demux_scores / demultiplex / trim_reads (csrc/wn_demux.hip through wavenet_speech_amd.demux) against the reference of
tests/demux_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality, ties included; the inputs
and their references are built once in tests/demux_cases.py, and tests/test_demux_ref.py holds the reference itself on the CPU."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import demux_cases as C
from tests import demux_ref as R
from tests.gpu_labels import INT_MIN, assert_pick as _assert_pick, assert_scores as _assert_scores, kit as _kit, kw as _kw
from tests.gpu_util import DEV, dev as _dev

pytestmark = pytest.mark.gpu


def test_the_case_worked_by_hand():
    case = C.CASES["hand"]
    got = W.demux_scores(_dev(case.labels), _dev(case.lengths), _kit(case), **_kw(case))
    assert got.score.tolist() == [[3.0, 1.0]] and got.start.tolist() == [[1, 2]] and got.end.tolist() == [[4, 5]]
    W.check_device_flags()


@pytest.mark.parametrize("name", [n for n in C.CASES if n != "hand"])
def test_cases_of_the_cpu_file(name):
    """P = 1; window = 1; patterns longer than the window; a read of length 0; reads shorter than the window; 1, 63, 64 and 65
    patterns per end, one end only, mixed lengths in a wave; the longest pattern on both sides of 8, 32, 64 and 96 rows, 128 rows at a
    window of 512; ties all the way; two labels; costs at +-1024 at the largest shape, ge = 0, go = ge, free gaps, a negative match"""
    case, ref = C.CASES[name], C.reference(name)
    _assert_scores(W.demux_scores(_dev(case.labels), _dev(case.lengths), _kit(case), **_kw(case)), ref)
    W.check_device_flags()


def test_forms_of_the_label_rows():
    """strided rows are read in place; int64 labels; int64 lengths; a list of lengths"""
    case, ref = C.CASES["rows_33"], C.reference("rows_33")
    kit, kw = _kit(case), _kw(case)
    B, L = case.labels.shape
    wide = torch.full((B, L + 5), 3, dtype=torch.int32, device=DEV)
    wide[:, :L] = _dev(case.labels)
    view = wide[:, :L]
    assert not view.is_contiguous()
    _assert_scores(W.demux_scores(view, _dev(case.lengths), kit, **kw), ref)
    _assert_scores(W.demux_scores(_dev(case.labels).long(), _dev(case.lengths).long(), kit, **kw), ref)
    _assert_scores(W.demux_scores(_dev(case.labels), case.lengths.tolist(), kit, **kw), ref)
    W.check_device_flags()


def test_a_poisoned_read_length():
    """a length below 0 and one above the row: their rows are INT_MIN / -1 / -1, counted entry by entry; the neighbours are untouched"""
    case, ref = C.CASES["k_63_65"], C.reference("k_63_65")
    labels = np.concatenate([case.labels, case.labels], 0)
    lengths = np.array([case.lengths[0], -1, case.lengths[0], case.labels.shape[1] + 1], dtype=np.int32)
    want = R.demux_scores_ref(labels, lengths, case.patterns, case.pattern_lengths, case.n_front, case.window, *case.costs)
    K = len(case.group)
    assert want["bad"] == 2 * K and np.array_equal(want["score"][0], ref["score"][0]) and (want["score"][[1, 3]] == INT_MIN).all()
    W.check_device_flags()
    got = W.demultiplex(_dev(labels), _dev(lengths), _kit(case), **_kw(case))
    assert np.array_equal(got.scores.start.cpu().numpy(), want["start"]) and np.array_equal(got.scores.end.cpu().numpy(), want["end"])
    assert got.scores.score[[1, 3]].eq(-2.0 ** 30).all() and torch.equal(got.scores.score[0], got.scores.score[2])
    assert got.hits[[1, 3]].eq(-1).all() and got.barcode[[1, 3]].eq(-1).all() and got.runner_up[[1, 3]].eq(INT_MIN).all()
    with pytest.raises(RuntimeError, match="%d \\(read, pattern\\) entries" % (2 * K)):
        W.check_device_flags()
    W.check_device_flags()


def test_a_poisoned_pattern_length():
    """through the C ABI (a BarcodeSet refuses such a table): lengths 0 and max_pattern_len + 1 poison their columns only"""
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    case = C.CASES["rows_9"]
    plen = case.pattern_lengths.copy()
    plen[1], plen[6] = 0, 9
    max_pat = 8
    want = R.demux_scores_ref(case.labels, case.lengths, case.patterns, plen, case.n_front, case.window, *case.costs, max_pattern_len=max_pat)
    B, K = want["score"].shape
    poisoned = np.array([not 1 <= int(P) <= max_pat for P in plen])
    assert poisoned.sum() == 4 and want["bad"] == 4 * B and (want["score"][:, poisoned] == INT_MIN).all() and (want["score"][:, ~poisoned] != INT_MIN).all()
    t = [_dev(a) for a in (case.labels, case.lengths, case.patterns, plen)]
    out = [torch.empty(B, K, dtype=torch.int32, device=DEV) for _ in range(3)]
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().wn_demux_scores(_p(t[0]), t[0].stride(0), _p(t[1]), _p(t[2]), t[2].stride(0), _p(t[3]), B, t[0].shape[1], K, case.n_front,
                                           max_pat, case.window, *case.costs, _p(out[0]), _p(out[1]), _p(out[2]), _p(bad), _stream()), "wn_demux_scores")
    torch.cuda.synchronize()
    for got, name in zip(out, ("score", "start", "end")):
        assert np.array_equal(got.cpu().numpy(), want[name]), name
    assert int(bad[0]) == want["bad"]


def test_the_planted_run():
    """64 reads, 12 barcodes at both ends, 8 % errors, seven reads missing one end: demultiplex equals the reference in every field
    (that the reference calls the truth is tests/test_demux_ref.py's), and trim_reads -> fastq_records prints the sliced strings"""
    p = C.planted()
    case = p["case"]
    scores, want = C.planted_reference()
    codes = ["".join(W.decoding.DEFAULT_ALPHABET[v] for v in c) for c in p["codes"]]
    kit = W.BarcodeSet(codes)
    assert np.array_equal(kit.patterns, case.patterns) and np.array_equal(kit.pattern_group, case.group) and kit.n_front == case.n_front
    labels, lengths = _dev(case.labels), _dev(case.lengths)
    got = W.demultiplex(labels, lengths, kit, window=C.PLANT_WINDOW, min_fraction=C.PLANT_FRACTION, min_margin=C.PLANT_MARGIN)
    _assert_scores(got.scores, scores)
    _assert_pick(got, want)
    assert got.names() == ["barcode%02d" % (g + 1) if g >= 0 else "unclassified" for g in want["barcode"].tolist()]
    qual = (torch.arange(case.labels.shape[1], device=DEV)[None, :] + torch.arange(len(case.lengths), device=DEV)[:, None]) % 94
    seq, n, q = W.trim_reads(labels, lengths, got.trim, qual=qual.to(torch.uint8))
    names = ["read%d" % b for b in range(len(case.lengths))]
    text = {0: ""}
    text.update({i: ch for i, ch in enumerate(W.decoding.DEFAULT_ALPHABET) if i})
    sliced = []
    for b, row in enumerate(p["seqs"]):
        t0, t1 = want["trim"][b]
        sliced.append("@read%d\n%s\n+\n%s\n" % (b, "".join(text[v] for v in row[t0:t1]), "".join(chr((j + b) % 94 + 33) for j in range(t0, t1))))
    assert W.fastq_records(names, seq, n, q) == sliced
    # require_both, and a margin that nothing clears
    both = W.demultiplex(labels, lengths, kit, window=C.PLANT_WINDOW, min_fraction=C.PLANT_FRACTION, min_margin=C.PLANT_MARGIN, require_both=True)
    floors = C.min_scores(case, 3, 5)
    _assert_pick(both, R.demux_pick_ref(scores["score"], scores["start"], scores["end"], case.lengths, case.group, floors, case.n_front, 12, True))
    none = W.demultiplex(labels, lengths, kit, window=C.PLANT_WINDOW, min_fraction=C.PLANT_FRACTION, min_margin=400.0)
    _assert_pick(none, R.demux_pick_ref(scores["score"], scores["start"], scores["end"], case.lengths, case.group, floors, case.n_front, 800, False))
    assert none.barcode.eq(-1).all() and not both.barcode.eq(-1).all() and not torch.equal(both.barcode, got.barcode)
    W.check_device_flags()


def test_pick_ties_and_groups_on_the_device():
    """the hand-made rules again, on the device: 65 patterns per end with many equal scores (ties to the lower index across the wave's
    stride), groups shared by several patterns"""
    case = C.CASES["k_63_65"]
    group = (np.arange(len(case.group)) % 5).astype(np.int32)
    ends = [0] * case.n_front + [1] * (len(group) - case.n_front)
    kit = W.BarcodeSet.from_table(case.patterns, case.pattern_lengths, ends, group)
    ref = C.reference("k_63_65")
    for fraction, num, den, margin in ((0.0, 0, 1, 0.0), (0.5, 1, 2, 1.0), (1.0, 1, 1, 0.0)):
        got = W.demultiplex(_dev(case.labels), _dev(case.lengths), kit, min_fraction=fraction, min_margin=margin, **_kw(case))
        want = R.demux_pick_ref(ref["score"], ref["start"], ref["end"], case.lengths, group, C.min_scores(case, num, den), case.n_front,
                                int(2 * margin), False)
        _assert_pick(got, want)
    W.check_device_flags()


def test_repeatable_and_captured():
    p = C.planted()
    case = p["case"]
    _, want = C.planted_reference()
    kit = _kit(case)
    labels, lengths = _dev(case.labels), _dev(case.lengths)
    a, b = (W.demux_scores(labels, lengths, kit, window=C.PLANT_WINDOW) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(a, b))              # two runs are bitwise identical
    kw = dict(window=C.PLANT_WINDOW, min_fraction=C.PLANT_FRACTION, min_margin=C.PLANT_MARGIN)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        eager = W.demultiplex(labels, lengths, kit, **kw)            # warms the allocator and uploads the tables on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = W.demultiplex(labels, lengths, kit, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _assert_pick(captured, want)
    for u, v in zip(captured[:4] + tuple(captured.scores), eager[:4] + tuple(eager.scores)):
        assert torch.equal(u, v)
    W.check_device_flags()


def test_reverse_complement_on_the_device():
    case = C.planted()["case"]
    labels, lengths = _dev(case.labels), _dev(case.lengths)
    rc = W.reverse_complement(labels, lengths)
    want = np.zeros_like(case.labels)
    for b, row in enumerate(C.planted()["seqs"]):
        want[b, :len(row)] = C.revcomp(row)
    assert rc.is_cuda and np.array_equal(rc.cpu().numpy(), want)
