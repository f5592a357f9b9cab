"""GPU: signal_map and map_reference (csrc/wn_sigmap.hip through wavenet_speech_amd.mapping) against the reference of
tests/signal_map_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality, ties included; the
inputs and their references are built once in tests/signal_map_cases.py.  The integer model of a case goes in as a hand-filled
SignalModel."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import signal_align_ref as AR
from tests import signal_map_cases as C
from tests import signal_map_ref as R
from tests.gpu_signal import assert_signal_mapping as _assert_equal, model_of as _model
from tests.gpu_util import DEV, dev as _dev, strided as _strided

pytestmark = pytest.mark.gpu


I64_MIN = np.iinfo(np.int64).min


_REFERENCES = {}


def _reference(name, case):
    """the prepared reference of a named case, made once (it is never changed by a call)"""
    if name not in _REFERENCES:
        _REFERENCES[name] = W.map_reference(torch.from_numpy(case.ref), _model(case), both_strands=False, device=DEV)
    return _REFERENCES[name]


def _call(name, case, signal=None, scale_shift=None, strip=None, want_end_cost=True):
    signal = _dev(case.signal) if signal is None else signal
    return W.signal_map(signal, _dev(case.signal_lengths), _reference(name, case), max_cost=case.kw["max_cost"], strip=strip,
                        scale_shift=None if scale_shift is None else _dev(scale_shift), want_end_cost=want_end_cost)


@pytest.mark.parametrize("M", C.SWEEP_M)
def test_size_sweep(M):
    """M around the block (64) and the tile (1024) and their multiples, T in {1, 2, 3, 65, 700} as the reads of one batch: the
    whole last row, the block table, score / end / start / runner_up"""
    name = "sweep_%d" % M
    case, ref = C.CASES[name], C.reference(name)
    got = _call(name, case)
    assert ref["bad"] == 0 and ref["ref_bad"] == 0
    _assert_equal(got, ref)
    W.check_device_flags()


def test_no_output_depends_on_the_strip():
    """M = 4100, T_b from 1 to 700: at strip 64 and T = 700 the halo spans a tile seam and every path crosses strip seams; at
    strip 2048 a workgroup sweeps three tiles and at 4160 (one strip) five, so the boundary column in LDS is rewritten in place"""
    case, ref = C.CASES["strips"], C.reference("strips")
    runs = [_call("strips", case, strip=s) for s in C.STRIPS + (2048, 4160)]
    for got in runs:
        _assert_equal(got, ref)
        assert all(torch.equal(u, v) for u, v in zip(got, runs[0]))
    W.check_device_flags()


@pytest.mark.parametrize("name", ["hand", "homopolymer", "two_copies", "seam_walls", "all_walls", "few_open_states", "t_above_m", "cost_clamp"])
@pytest.mark.parametrize("strip", [64, 576, None])
def test_ties_walls_and_edges(name, strip):
    """the case worked by hand; every cell equal; two copies of a locus in different strips and tiles (the left one wins); walls on
    strip and tile seams; a reference that is all walls (no mapping); fewer open states than samples; T_b above M; the cost clamp"""
    case, ref = C.CASES[name], C.reference(name)
    got = _call(name, case, strip=strip)
    _assert_equal(got, ref)
    if name == "all_walls":
        assert (got.end == -1).all() and (got.score == 2 ** 63 - 1).all() and (got.strand == -1).all()
        labels, lengths = got.labels()
        assert tuple(labels.shape) == (2, 1) and lengths.tolist() == [0, 0] and got.ref_span().tolist() == [[-1, -1]] * 2
    W.check_device_flags()


@pytest.mark.parametrize("k", [1, 5, 6])
def test_input_forms(k):
    """k in {1, 5, 6}: float32 contiguous, row-strided, [B, 1, L]; int16 with scale_shift; end_cost on and off"""
    name = "form_k%d" % k
    case, ref = C.CASES[name], C.reference(name)
    _assert_equal(_call(name, case, want_end_cost=False), ref, end_cost=False)
    _assert_equal(_call(name, case, signal=_strided(case.signal, False)), ref)
    _assert_equal(_call(name, case, signal=_strided(case.signal, True), strip=128), ref)
    raw, ss = C.int16_form(name)
    want = C.int16_reference(name)
    assert want["bad"] == 0
    _assert_equal(_call(name, case, signal=_dev(raw), scale_shift=ss), want)
    _assert_equal(_call(name, case, signal=_strided(raw, True), scale_shift=ss, want_end_cost=False), want, end_cost=False)
    W.check_device_flags()


def test_bad_reads_among_good_ones():
    case, ref = C.bad_batch(), C.bad_reference()
    W.check_device_flags()
    got = _call("bad_batch", case, strip=128)
    _assert_equal(got, ref)
    bad = np.array([name not in C.BAD_GOOD for name in C.BAD_READS])
    assert ref["bad"] == int(bad.sum()) == 5
    for t in (got.score, got.runner_up, got.block_cost, got.end_cost):
        assert (t.cpu().numpy()[bad] == I64_MIN).all()
    for t in (got.end, got.start, got.block_end):
        assert (t.cpu().numpy()[bad] == -1).all()
    with pytest.raises(RuntimeError, match="5 bad read"):
        W.check_device_flags()
    for b in np.flatnonzero(~bad):                                   # the good reads are what they are alone
        alone = C.Case(case.signal[b:b + 1], case.signal_lengths[b:b + 1], case.ref, case.model, case.kw, None)
        one = _call("bad_batch", alone)
        assert all(torch.equal(u[0], v[b]) for u, v in zip(one, got))
    W.check_device_flags()


def test_faults_of_the_reference_are_counted_and_mapped_as_walls():
    case = C.faulty_reference_case()
    ref = C.call_ref(case)
    W.check_device_flags()
    reference = W.map_reference(torch.from_numpy(case.ref), _model(case), both_strands=False, device=DEV)
    with pytest.raises(RuntimeError, match="%d fault" % ref["ref_bad"]):
        W.check_device_flags()
    assert ref["ref_bad"] > 1
    got = W.signal_map(_dev(case.signal), _dev(case.signal_lengths), reference, want_end_cost=True)
    _assert_equal(got, ref)
    W.check_device_flags()


def test_round_trip_on_the_fixture():
    """the 24 reads of both strands (generated on the CPU, moved to the device): the mapping equals the reference and costs no more
    than the true path; signal_align on labels() (band 2048, wider than any span: unbanded) finds the same score; its starts drive
    kmer_events with no bad read"""
    fx, ref = C.fixture(), C.fixture_reference()
    model = fx["model"]
    reference = W.map_reference(torch.from_numpy(fx["bases"]), model, device=DEV)
    assert (reference.R, reference.ref_len, reference.k, reference.n_states) == (3000, 6001, 5, 5997)
    assert np.array_equal(reference.bases.cpu().numpy(), fx["joined"])
    signal, lengths = _dev(fx["signal"]), _dev(fx["signal_lengths"])
    got = W.signal_map(signal, lengths, reference, want_end_cost=True)
    _assert_equal(got, ref)
    W.check_device_flags()
    assert got.strand.cpu().tolist() == fx["strand"].tolist()
    assert (np.abs(got.start.cpu().numpy() - fx["start_state"]) <= 2).all()
    span = got.ref_span().cpu().tolist()
    assert span == [list(R.ref_span_of(int(s), int(e), 3000, 5)) for s, e in zip(ref["start"], ref["end"])]
    tab = model.table.numpy().astype(np.int64)
    sample_kmer = fx["reads"].sample_kmer.numpy()
    for b in range(24):                                              # the true path is one of the paths
        T = int(fx["signal_lengths"][b])
        q = np.array(AR.read_samples(fx["signal"][b], T, None, model.frac_bits), dtype=np.int64)
        codes = np.array(AR.read_states(fx["read_bases"][b], 120, 5, 0), dtype=np.int64)
        rows = tab[codes[sample_kmer[b, :T]]]
        true_cost = int(AR.cost_row(q, rows[:, 0], rows[:, 1], rows[:, 2], model.weight_shift, 2 ** 31 - 1).sum())
        assert int(got.score[b]) <= true_cost, b
    labels, label_lengths = got.labels()
    assert labels.dtype == torch.int32 and label_lengths.tolist() == (ref["end"] - ref["start"] + 5).tolist()
    for b in range(24):
        s, n = int(ref["start"][b]), int(label_lengths[b])
        assert labels[b, :n].cpu().tolist() == fx["joined"][s:s + n].tolist() and not bool(labels[b, n:].any())
    al = W.signal_align(signal, lengths, labels, label_lengths, model, first=0, band=2048)
    assert torch.equal(al.score, got.score) and not bool(al.band_hits.any())
    ev = W.kmer_events(signal, lengths, labels, label_lengths, starts=al.starts, k=al.k, first=al.first)
    W.check_device_flags()                                           # no bad read
    assert torch.equal(ev.read_counts[:, 3], lengths) and torch.equal(ev.read_counts[:, 0], label_lengths - 4)
    nats = got.nats.cpu()
    assert nats.dtype == torch.float64 and float(nats[0]) == int(got.score[0]) / 256.0


def test_repeatable_and_captured():
    case, ref = C.CASES["strips"], C.reference("strips")
    a, b = _call("strips", case), _call("strips", case)
    assert all(torch.equal(u, v) for u, v in zip(a, b))              # two runs are bitwise identical
    args = [_dev(case.signal), _dev(case.signal_lengths), _reference("strips", case)]
    kw = dict(want_end_cost=True, strip=576)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        W.signal_map(*args, **kw)                                    # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = W.signal_map(*args, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(captured, ref)
    assert all(torch.equal(u, v) for u, v in zip(captured, a))
    W.check_device_flags()
