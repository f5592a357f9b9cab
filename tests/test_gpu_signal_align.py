"""GPU: signal_align (csrc/wn_sigalign.hip through wavenet_speech_amd.signal_align) against the reference of
tests/signal_align_ref.py.  Everything the kernel writes is an integer, so every comparison is exact equality, ties included; the
inputs and their references are built once in tests/signal_align_cases.py.  The integer model of a case goes in as a hand-filled
SignalModel."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import signal_align_cases as C
from tests import signal_align_ref as R
from tests.gpu_signal import assert_signal_alignment as _assert_equal, model_of as _model
from tests.gpu_util import dev as _dev, strided as _strided
from wavenet_speech_amd import synthetic as S

pytestmark = pytest.mark.gpu


def _call(case, signal=None, scale_shift=None, want_states=True, band=None, labels=None):
    kw = case.kw
    signal = _dev(case.signal) if signal is None else signal
    return W.signal_align(signal, _dev(case.signal_lengths), _dev(case.labels) if labels is None else labels, _dev(case.label_lengths),
                          _model(case), first=kw["first"], band=band or kw["band"], max_cost=kw["max_cost"],
                          scale_shift=None if scale_shift is None else _dev(scale_shift), want_states=want_states)


SMALL = ["hand", "small", "band_never_moves", "moving_band", "sample_chunk_edges", "homopolymer", "dyadic", "cost_clamp",
         "threads_w64", "threads_w512", "threads_w576", "threads_w2048", "pressed_w64", "pressed_w2048", "long_read"]


@pytest.mark.parametrize("name", SMALL)
def test_against_the_reference(name):
    """the hand case; N = 1, N = T, T = N - 1, T = 0, labels shorter than k + 2 first; a band that never moves and one whose slots
    wrap; T around the kernel's sample chunk; ties; the cost clamp; 8 to 256 threads at work; a path pressed against the band; a
    read of 70 000 samples"""
    case, ref = C.CASES[name], C.reference(name)
    got = _call(case)
    assert ref["bad"] == 0
    _assert_equal(got, ref)
    assert (got.k, got.first, got.frac_bits, got.band) == (case.kw["k"], case.kw["first"], case.kw["frac_bits"], case.kw["band"])
    W.check_device_flags()


def test_band_wide_enough_is_the_unbanded_optimum():
    case = C.CASES["band_never_moves"]
    free = C.call_ref(case, band=None)
    got = _call(case)
    assert got.score.cpu().tolist() == free["score"].tolist() and np.array_equal(got.states.cpu().numpy(), free["states"])
    assert int(got.band_hits[0]) == 0


def test_path_pressed_against_the_band():
    tight, wide = _call(C.CASES["pressed_w64"]), _call(C.CASES["pressed_w2048"])
    assert int(tight.band_hits[0]) > 0 and int(wide.band_hits[0]) == 0
    assert int(wide.score[0]) <= int(tight.score[0])
    nats = tight.nats.cpu()
    assert nats.dtype == torch.float64 and float(nats[0]) == int(tight.score[0]) / 256.0


@pytest.mark.parametrize("name", sorted(n for n in C.CASES if n.startswith("form_")))
def test_input_forms(name):
    """k in {1, 5, 6} x first in {0, 2}: float32 contiguous, row-strided, [B, 1, L]; int16 with scale_shift; int64 labels; states on
    and off"""
    case, ref = C.CASES[name], C.reference(name)
    _assert_equal(_call(case, want_states=False), ref, states=False)
    _assert_equal(_call(case, signal=_strided(case.signal, False)), ref)
    _assert_equal(_call(case, signal=_strided(case.signal, True), labels=_dev(case.labels.astype(np.int64))), ref)
    raw, ss = C.int16_form(name)
    want = C.int16_reference(name)
    assert want["bad"] == 0
    _assert_equal(_call(case, signal=_dev(raw), scale_shift=ss), want)
    _assert_equal(_call(case, signal=_strided(raw, True), scale_shift=ss, want_states=False), want, states=False)
    W.check_device_flags()


def test_bad_reads_among_good_ones():
    case, ref = C.bad_batch(), C.bad_reference()
    W.check_device_flags()
    got = _call(case)
    _assert_equal(got, ref)
    bad = np.array([name not in C.BAD_GOOD for name in C.BAD_READS])
    assert ref["bad"] == int(bad.sum()) == 10
    score = got.score.cpu().numpy()
    assert (score[bad] == np.iinfo(np.int64).min).all() and (np.abs(score[~bad]) < 2 ** 40).all()
    assert (got.starts.cpu().numpy()[bad] == -1).all() and (got.states.cpu().numpy()[bad] == -1).all()
    assert (got.band_hits.cpu().numpy()[bad] == -1).all()
    with pytest.raises(RuntimeError, match="10 bad read"):
        W.check_device_flags()
    # the good reads are what they are alone, whatever their neighbours
    for b in np.flatnonzero(~bad):
        alone = C.Case(case.signal[b:b + 1], case.signal_lengths[b:b + 1], case.labels[b:b + 1], case.label_lengths[b:b + 1], case.model,
                       case.kw, None)
        one = _call(alone)
        assert torch.equal(one.starts[0], got.starts[b]) and int(one.score[0]) == int(got.score[b])
        assert torch.equal(one.states[0], got.states[b])
    W.check_device_flags()
    # int16: no NaN to meet, but a scale that carries a sample out of range and a non-finite shift, with a good read between
    raw = np.rint(case.signal[:1] * 8.0).astype(np.int16).repeat(3, 0)
    ss = np.array([[40.0, 0.0], [0.125, 0.0], [0.125, np.inf]], dtype=np.float32)
    sub = C.Case(raw, case.signal_lengths[:1].repeat(3), case.labels[:1].repeat(3, 0), case.label_lengths[:1].repeat(3), case.model, case.kw,
                 None)
    want = C.call_ref(sub, scale_shift=ss)
    assert want["bad"] == 2 and want["score"][1] not in (R.BAD_READ, R.NO_ALIGNMENT)
    _assert_equal(_call(sub, scale_shift=ss), want)
    with pytest.raises(RuntimeError, match="2 bad read"):
        W.check_device_flags()


def test_repeatable_and_captured():
    case, ref = C.CASES["moving_band"], C.reference("moving_band")
    a, b = _call(case), _call(case)
    assert all(torch.equal(u, v) for u, v in zip(a, b))              # two runs are bitwise identical
    model = _model(case)
    args = [_dev(case.signal), _dev(case.signal_lengths), _dev(case.labels), _dev(case.label_lengths), model]
    kw = dict(first=case.kw["first"], band=case.kw["band"], want_states=True)
    W.signal_align(*args, **kw)                                      # the model's table is on the device from here on
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        W.signal_align(*args, **kw)                                  # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = W.signal_align(*args, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(captured, ref)
    assert all(torch.equal(u, v) for u, v in zip(captured, a))
    W.check_device_flags()


def test_round_trip_with_the_generator():
    """128 generated reads, dwell uniform in [4, 8), loader window, the stand-in table, band 64.  The true segmentation lies inside
    the band (asserted from the generator's starts alone), so the alignment may not cost more than it; its starts drive kmer_events
    with no bad read.  The share of samples put in their true k-mer is printed, not asserted: nothing derives it."""
    table = S.standin_kmer_table()
    model = W.signal_model(*table)
    g = torch.Generator().manual_seed(5)
    reads = S.ragged_reads(128, (200, 300), ("uniform", 6, 2), "loader", table, generator=g, device="cuda", pad_to=None)
    band = 64
    starts = reads.starts.cpu().numpy().astype(np.int64)
    lengths, n_states = reads.signal_lengths.cpu().numpy(), reads.base_lengths.cpu().numpy() - 8
    sample_kmer = reads.sample_kmer.cpu().numpy()
    for b in range(128):                                             # a condition on the input, not on the kernel
        T, N = int(lengths[b]), int(n_states[b])
        assert starts[b, N] == T and T >= N
        t = np.arange(T)
        lo = np.clip(((2 * t + 1) * N) // (2 * T) - band // 2, 0, max(N - band, 0))
        true = sample_kmer[b, :T]
        assert ((lo <= true) & (true < lo + band)).all(), b
    al = W.signal_align(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, model, first=2, band=band, want_states=True)
    W.check_device_flags()
    assert tuple(al.starts.shape) == tuple(reads.starts.shape)
    score = al.score.cpu().tolist()
    signal, bases = reads.signal[:, 0].cpu().numpy(), reads.bases.cpu().numpy()
    tab = model.table.numpy().astype(np.int64)
    for b in range(128):
        T, N = int(lengths[b]), int(n_states[b])
        q = np.array(R.read_samples(signal[b], T, None, 12), dtype=np.int64)
        codes = np.array(R.read_states(bases[b], N + 8, 5, 2), dtype=np.int64)
        rows = tab[codes[sample_kmer[b, :T]]]
        true_cost = int(R.cost_row(q, rows[:, 0], rows[:, 1], rows[:, 2], model.weight_shift, 2 ** 31 - 1).sum())
        assert score[b] <= true_cost, b
        if b < 4:                                                    # and the score is the cost of the segmentation it returns
            assert R.rescore(q.tolist(), codes.tolist(), tab, model.weight_shift, 2 ** 31 - 1, al.starts[b].cpu().tolist()) == score[b]
    ev = W.kmer_events(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, starts=al.starts, k=al.k, first=al.first)
    W.check_device_flags()                                           # no bad read
    assert torch.equal(ev.read_counts[:, 0].long(), reads.base_lengths.long() - 8)
    assert torch.equal(ev.read_counts[:, 3], reads.signal_lengths.int())
    inside = reads.sample_kmer >= 0
    agree = float((al.states == reads.sample_kmer)[inside].double().mean())
    print("samples in their true k-mer: %.4f of %d; band hits %d" % (agree, int(inside.sum()), int(al.band_hits.sum())))
