"""GPU: event_align (csrc/wn_eventalign.hip through wavenet_speech_amd.events) against the reference of tests/event_align_ref.py.
Everything the kernel writes is an integer, so every comparison is exact equality, ties included; the inputs and their references
are built once in tests/event_align_cases.py, and tests/test_event_align_ref.py holds the reference itself on the CPU."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import event_align_cases as C
from tests import event_align_ref as R
from tests.gpu_signal import assert_event_alignment as _assert_equal, assert_move_counts as _assert_counts, event_align as _call
from tests.gpu_signal import event_model as _model, event_tables as _events
from tests.gpu_util import DEV, dev as _dev

pytestmark = pytest.mark.gpu


def test_the_case_worked_by_hand():
    """three events over four states, one boundary missed: 103, and of the two paths that cost it the one with the smaller last move"""
    got = _call(C.CASES["hand"])
    assert got.score.tolist() == [103] and got.states.tolist() == [[0, 2, 3, -1, -1]]
    assert got.starts.tolist() == [[0, 2, 2, 4, 5]] and got.moves.tolist() == [[0, 1, 1, 0]] and got.band_hits.tolist() == [0]
    assert (got.k, got.first, got.frac_bits, got.cost_bits, got.band, got.move_costs) == (1, 0, C.F, C.COST_BITS, 64, (3, 1, 2, 40))
    assert got.nats.tolist() == [103 / 256.0]
    W.check_device_flags()


SHAPES = ["homopolymer", "noisy", "one_event", "one_state", "all_double_skips", "one_state_too_many", "tile_255", "tile_256", "tile_257",
          "tile_512", "every_slot_reused", "three_rearm", "threads_w64", "threads_w512", "threads_w576", "threads_w2048", "forbid_no_stay",
          "forbid_no_skip", "forbid_no_double_skip", "forbid_no_single_skip"] + ["limit_%d" % i for i in range(8)]


@pytest.mark.parametrize("name", SHAPES)
def test_cases_of_the_cpu_file(name):
    """ties on a homopolymer; fewer events than states; E = 1; N = 1 (all stays); N = 3 (E - 1) + 1 (all double skips) and one state
    more (no alignment); E on either side of the event tile and at twice its size; every slot reused; three slots re-armed per step;
    one, one, two and four waves at N = 2200; each move forbidden in turn; events of 65536 samples at +-(2^23 - 1) with the clamp on
    both sides"""
    case, ref = C.CASES[name], C.reference(name)
    got = _call(case)
    _assert_equal(got, ref)
    _assert_counts(got, case, ref)
    W.check_device_flags()


def test_what_the_shapes_reach():
    """conditions on the cases, from the references alone"""
    assert C.reference("one_state")["moves"].tolist() == [[39, 0, 0, 0]]
    assert C.reference("all_double_skips")["moves"].tolist() == [[0, 0, 0, 49]]
    assert C.reference("one_state_too_many")["score"].tolist() == [R.NO_ALIGNMENT]
    assert [int(C.CASES["tile_%d" % E].n_events[0]) for E in (255, 256, 257, 512)] == [C.EVENT_TILE - 1, C.EVENT_TILE, C.EVENT_TILE + 1, 2 * C.EVENT_TILE]
    case = C.CASES["every_slot_reused"]
    assert case.n_events[0] >= 420 and C.reference("every_slot_reused")["moves"][0, 0] > 100
    case = C.CASES["three_rearm"]
    E, N = int(case.n_events[0]), int(case.label_lengths[0]) - 4
    assert (E, N) == (210, 610) and max(R.band_lo(e + 1, N, E, 64) - R.band_lo(e, N, E, 64) for e in range(E - 1)) == 3
    case = C.CASES["threads_w64"]
    assert case.n_events[0] < 2200 - 4 and C.reference("threads_w2048")["band_hits"].tolist() == [0]
    for name, m in (("forbid_no_stay", 0), ("forbid_no_skip", 2), ("forbid_no_skip", 3), ("forbid_no_double_skip", 3), ("forbid_no_single_skip", 2)):
        assert (C.reference(name)["moves"][:, m] == 0).all() and (C.reference(name)["score"] != R.NO_ALIGNMENT).all(), name


def test_a_path_pressed_against_the_band():
    narrow, wide = _call(C.CASES["pressed_w64"]), _call(C.CASES["pressed_w2048"])
    _assert_equal(narrow, C.reference("pressed_w64"))
    _assert_equal(wide, C.reference("pressed_w2048"))
    assert int(narrow.band_hits[0]) > 0 and int(wide.band_hits[0]) == 0 and int(wide.score[0]) <= int(narrow.score[0])
    W.check_device_flags()


@pytest.mark.parametrize("k,first", [(1, 0), (1, 2), (5, 0), (5, 2), (6, 0), (6, 2)])
def test_forms(k, first):
    """k and first; int64 labels; a row-strided label view; states on and off; a DetectedEvents in place of the tuple"""
    name = "form_k%d_first%d" % (k, first)
    case, ref = C.CASES[name], C.reference(name)
    _assert_equal(_call(case), ref)
    _assert_equal(_call(case, labels=_dev(case.labels).long(), states=False), ref, states=False)
    wide = torch.zeros(case.labels.shape[0], case.labels.shape[1] + 3, dtype=torch.int32, device=DEV)
    wide[:, :case.labels.shape[1]] = _dev(case.labels)
    _assert_equal(_call(case, labels=wide[:, :case.labels.shape[1]]), ref)
    ev = W.DetectedEvents(*_events(case), torch.zeros(case.ev_sum.shape, dtype=torch.int32, device=DEV), frac_bits=C.F)
    kw = case.kw
    got = W.event_align(ev, _dev(case.labels), _dev(case.label_lengths), _model(case), first=first, band=kw["band"], moves=kw["move_cost"],
                        want_states=True)
    _assert_equal(got, ref)
    W.check_device_flags()


def test_probabilities_become_the_costs_of_move_costs():
    case, ref = C.CASES["noisy"], C.reference("noisy")
    assert W.move_costs(W.DEFAULT_MOVES, C.COST_BITS) == C.MOVES
    got = _call(case, moves=W.DEFAULT_MOVES)
    _assert_equal(got, ref)
    assert got.move_costs == C.MOVES
    fit = W.fit_moves(got.moves)
    assert abs(sum(fit) - 1.0) < 1e-12 and fit == tuple(t / ref["moves"].sum() for t in ref["moves"].sum(0).tolist())
    W.check_device_flags()


def _raw_call(case, max_states):
    """through the C ABI, so that max_states can be smaller than the labels allow"""
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    lib = _lib.load()
    kw = case.kw
    B, M = len(case.n_events), case.ev_starts.shape[1] - 1
    t = [_dev(case.n_events), _dev(case.ev_starts), _dev(case.ev_sum), _dev(case.ev_sumsq), _dev(case.labels), _dev(case.label_lengths),
         _dev(case.model.astype(np.int32))]
    i32 = dict(dtype=torch.int32, device=DEV)
    starts, score = torch.empty(B, max_states + 1, **i32), torch.empty(B, dtype=torch.int64, device=DEV)
    states, moves, hits, bad = torch.empty(B, M, **i32), torch.empty(B, 4, **i32), torch.empty(B, **i32), torch.zeros(1, **i32)
    ws = torch.empty(lib.wn_event_align_workspace_bytes(B, M, kw["band"]), dtype=torch.uint8, device=DEV)
    mc = kw["move_cost"]
    _lib.check(lib.wn_event_align(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]), t[4].stride(0), _p(t[5]), _p(t[6]), B, M,
                                  int(t[4].shape[1]), max_states, kw["k"], kw["first"], C.F, kw["weight_shift"], 2 ** 31 - 1, kw["band"], mc[0],
                                  mc[1], mc[2], mc[3], _p(starts), _p(score), _p(states), _p(moves), _p(hits), _p(ws), ws.numel(), _p(bad),
                                  _stream()), "wn_event_align")
    torch.cuda.synchronize()
    return W.EventAlignment(starts, score, hits, moves, states), int(bad[0])


def test_faults_among_good_reads():
    """each length out of range both ways, N above max_states; labels 0 and 5 at the window's two ends, harmless ones just outside;
    n = 0, n = 65537, decreasing starts, |S| one over its bound, Q = -1, S^2 = n Q + 1, a model row with weight 0, a negative first
    start; garbage past a read's events is never read"""
    (case, max_states), ref = C.bad_batch(), C.bad_reference()
    bad = np.array([name not in C.BAD_GOOD for name in C.BAD_READS])
    assert ref["bad"] == int(bad.sum()) == 15 and [int(v) for v in ref["score"][bad]] == [R.BAD_READ] * 15
    got, counted = _raw_call(case, max_states)
    _assert_equal(got, ref)
    assert counted == 15
    for t in (got.starts, got.states, got.moves, got.band_hits):
        assert (t.cpu().numpy()[bad] == -1).all()
    for b in np.flatnonzero(~bad):                                   # the good reads are what they are alone
        alone = C.Case(*[f[b:b + 1] for f in case[:6]], case.model, case.kw, None)
        one, none_bad = _raw_call(alone, max_states)
        assert none_bad == 0 and all(torch.equal(u[0], v[b]) for u, v in zip(one, got))
    # and through the wrapper: the same batch without the two reads it cannot fault (max_states follows the labels' width, and a
    # SignalModel refuses a weight of 0 on the host), under the table as it was
    keep = np.array([name not in ("states_above", "weight_0") for name in C.BAD_READS])
    sub = C.Case(*[f[keep] for f in case[:6]], C.SC.table(C.BAD_K)[2], case.kw, None)
    W.check_device_flags()
    via = _call(sub)
    assert via.score.tolist() == [int(v) for v in ref["score"][keep]] and np.array_equal(via.moves.cpu().numpy(), ref["moves"][keep])
    with pytest.raises(RuntimeError, match="13 bad read"):
        W.check_device_flags()
    W.check_device_flags()


def test_repeatable_and_captured():
    case, ref = C.CASES["noisy"], C.reference("noisy")
    a, b = _call(case), _call(case)
    assert all(torch.equal(u, v) for u, v in zip(a, b))              # two runs are bitwise identical
    events, labels, ll, model = _events(case), _dev(case.labels), _dev(case.label_lengths), _model(case)
    kw = dict(first=case.kw["first"], band=case.kw["band"], moves=case.kw["move_cost"], want_states=True, frac_bits=C.F)
    model.on(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        W.event_align(events, labels, ll, model, **kw)               # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = W.event_align(events, labels, ll, model, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(captured, ref)
    assert all(torch.equal(u, v) for u, v in zip(captured, a))
    W.check_device_flags()


def test_composition_raw_noisy_reads_to_events_to_alignment_to_tables():
    """raw noisy reads -> detect_events -> event_align -> kmer_events(starts=al.starts): every read has fewer events than k-mers,
    so signal_align has no alignment for any; event_align aligns all of them, equal to the reference on the device's own event
    table, and the event tables use N - counts[2] - 2 counts[3] states per read, with no bad read"""
    fx = C.gap_reads()
    signal, lengths = _dev(fx["signal"]), _dev(fx["signal_lengths"])
    labels, ll = _dev(fx["labels"]), _dev(fx["label_lengths"])
    ev = W.detect_events(signal, lengths, frac_bits=C.F, max_events=256)
    n = C.GAP_STATES
    assert not bool(ev.truncated.any()) and bool((ev.n_events < n).all()) and bool((ev.n_events > n // 3 + 1).all())
    model = W.SignalModel(torch.from_numpy(C.gap_model(fx)), C.S, frac_bits=C.F, cost_bits=C.COST_BITS)
    means, counts = ev.as_signal()
    assert W.signal_align(means, counts, labels, ll, model, first=0, band=64).score.tolist() == [R.NO_ALIGNMENT] * C.GAP_READS
    al = W.event_align(ev, labels, ll, model, first=0, band=64, want_states=True)
    ref = R.event_align_ref(ev.n_events.cpu().numpy(), ev.starts.cpu().numpy(), ev.sum.cpu().numpy(), ev.sumsq.cpu().numpy(), fx["labels"],
                            fx["label_lengths"], C.gap_model(fx), C.MOVES, k=C.GAP_K, first=0, weight_shift=C.S, band=64)
    _assert_equal(al, ref)
    assert ref["bad"] == 0 and all(int(v) < R.INF for v in ref["score"])
    tables = W.kmer_events(signal, lengths, labels, ll, starts=al.starts, k=C.GAP_K, first=0)
    used = n - al.moves[:, 2] - 2 * al.moves[:, 3]
    assert torch.equal(tables.read_counts[:, 0], used) and torch.equal(tables.read_counts[:, 3], lengths)
    assert torch.equal((tables.kmer == -2).sum(1).int(), n - used)
    W.check_device_flags()


def test_wrapper_refusals_on_the_device():
    case = C.CASES["hand"]
    events, labels, ll, model = _events(case), _dev(case.labels), _dev(case.label_lengths), _model(case)
    for kw in (dict(band=32), dict(band=96), dict(band=4096), dict(first=-1), dict(first=9), dict(max_cost=0), dict(moves=(0.1, 0.0, 0.1, 0.1)),
               dict(moves=(0.1, 0.5, 0.1)), dict(moves=(5, -1, 5, 5)), dict(moves=(5, 5, -2, 5)), dict(moves=(5, 5, 2 ** 30, 5)),
               dict(frac_bits=C.F + 1), dict(frac_bits=None)):
        with pytest.raises(ValueError, match="event_align|move_costs"):
            W.event_align(events, labels, ll, model, **dict(dict(frac_bits=C.F), **kw))
    with pytest.raises(ValueError, match="event_align"):
        W.event_align(events[:3], labels, ll, model, frac_bits=C.F)
    with pytest.raises(ValueError, match="event_align"):
        W.event_align((events[0], events[1], events[2].int(), events[3]), labels, ll, model, frac_bits=C.F)
    with pytest.raises(ValueError, match="event_align"):
        W.event_align((events[0], events[1], events[2][:, :-1], events[3]), labels, ll, model, frac_bits=C.F)
    W.check_device_flags()
