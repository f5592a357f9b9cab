"""GPU: detect_events (csrc/wn_eventdetect.hip through wavenet_speech_amd.events) against the reference of
tests/event_detect_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality, ties included; the
inputs and their references are built once in tests/event_detect_cases.py, and tests/test_event_detect_ref.py shows on the CPU
what each case reaches."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import event_detect_cases as C
from tests.gpu_signal import assert_detected as _assert_equal, detect_events as _call
from tests.gpu_util import DEV, dev as _dev, strided as _strided

pytestmark = pytest.mark.gpu


def test_lengths_around_the_windows_and_the_seams():
    """T in {0, 1, 2w - 1, 2w, 2w + 1, 255, 256, 257, 511, 512, 513, 1100} as the ragged reads of one batch, chunk 256"""
    case, ref = C.CASES["lengths"], C.reference("lengths")
    got = _call(case)
    _assert_equal(got, ref)
    assert got.n_events.tolist()[:2] == [0, 1] and not bool(got.truncated.any())
    n = got.held.cpu()
    length, mean, stdv = got.length.cpu(), got.mean.cpu(), got.stdv.cpu()
    assert length.dtype == torch.int32 and torch.equal(length.sum(1), torch.from_numpy(case.signal_lengths).long())
    assert mean.dtype == torch.float64 and stdv.dtype == torch.float64
    b = len(C.LENGTHS) - 1
    q = np.rint(case.signal[b, :1100].astype(np.float64) * 4096.0)
    s0, s1 = int(got.starts[b, 3]), int(got.starts[b, 4])
    assert float(mean[b, 3]) == q[s0:s1].sum() / ((s1 - s0) * 4096.0) and abs(float(stdv[b, 3]) - q[s0:s1].std() / 4096.0) < 1e-9
    assert bool(torch.isnan(mean[b, int(n[b]):]).all())
    means, lengths = got.as_signal()
    assert means.dtype == torch.float32 and lengths.dtype == torch.int32 and torch.equal(lengths.cpu(), n.int())
    assert not bool(torch.isnan(means).any()) and float(means[b, 3]) == float(mean[b, 3].float())
    W.check_device_flags()


def test_no_output_depends_on_the_chunk():
    case, ref = C.CASES["lengths"], C.reference("lengths")
    runs = [_call(case, chunk=c) for c in (256, 1024, None, 768, 16384)]
    for got in runs:
        _assert_equal(got, ref)
        assert all(torch.equal(u, v) for u, v in zip(got, runs[0]))
    W.check_device_flags()


@pytest.mark.parametrize("name", ["seams", "halo", "merge", "ties", "width", "noise_free", "forced_small", "forced_gap_64", "forced_gap_5"])
@pytest.mark.parametrize("chunk", [256, None])
def test_cases_of_the_cpu_file(name, chunk):
    """a peak on a chunk seam, one sample either side, a short / long pair across it; the merge distance; ties; the comparator's
    width; noise-free recovery; forced splits of max_event_len = 64 on 3 * 64 + 5, 64 and 65 constant samples, and of 64 and 5 in
    gaps long enough for the workgroup's shared list, before a boundary and before the read's end"""
    case, ref = C.CASES[name], C.reference(name)
    got = _call(case, chunk=chunk)
    _assert_equal(got, ref)
    if case.truth is not None:
        dev = dict(n_events=got.n_events.cpu().numpy(), starts=got.starts.cpu().numpy(), kind=got.kind.cpu().numpy())
        assert [C.boundaries(dev, b) for b in range(len(case.truth))] == case.truth
    W.check_device_flags()


@pytest.mark.parametrize("M", [1, 2, 3])
def test_many_forced_splits_inside_one_word(M):
    """max_event_len 1, 2, 3 on 66000-sample reads with a boundary every 18..60 samples: gaps inside one 64-position word with 17
    to 59 forced splits, thousands per 1024-word step of the ranks launch, in more than one step"""
    case, ref = C.CASES["dense_%d" % M], C.reference("dense_%d" % M)
    got = _call(case, chunk=None)
    _assert_equal(got, ref)
    assert got.n_events.tolist() == [-(-C.DENSE_T // M)] * 3 if M == 1 else int(got.n_events.min()) > C.DENSE_T // (M + 1)
    W.check_device_flags()


def test_forced_splits_at_the_largest_event():
    """max_event_len = 65536 on constant reads of +-(2^23 - 1), T = 2 * 65536 + 3: sums of squares near 2^62, in closed form"""
    case, ref = C.CASES["forced_large"], C.reference("forced_large")
    got = _call(case, chunk=None)
    _assert_equal(got, ref)
    m = C.QMAX
    assert got.sumsq[:, :3].tolist() == [[65536 * m * m, 65536 * m * m, 3 * m * m]] * 2
    assert got.sum[:, :3].tolist() == [[65536 * m, 65536 * m, 3 * m], [-65536 * m, -65536 * m, -3 * m]]
    assert got.starts[0].tolist() == [0, 65536, 131072] + [131075] * 6 and got.kind[1].tolist() == [0, 3, 3] + [-1] * 5
    W.check_device_flags()


def test_truncation_keeps_the_true_count_and_whole_events():
    case, ref, full = C.CASES["truncated"], C.reference("truncated"), C.reference("lengths")
    got = _call(case)
    _assert_equal(got, ref)
    assert got.max_events == 7 and np.array_equal(got.n_events.cpu().numpy(), full["n_events"])
    assert got.truncated.tolist() == (full["n_events"] > 7).tolist() and bool(got.truncated.any()) and not bool(got.truncated.all())
    b = len(C.LENGTHS) - 1
    assert got.starts[b].tolist() == full["starts"][b, :8].tolist() and got.sum[b].tolist() == [int(v) for v in full["sum"][b, :7]]
    assert got.held.tolist() == np.minimum(full["n_events"], 7).tolist()
    W.check_device_flags()


def test_input_forms():
    """float32 row-strided and [B, 1, L]; int16 with scale_shift, contiguous and as a strided [B, 1, L] view"""
    case, ref = C.CASES["lengths"], C.reference("lengths")
    _assert_equal(_call(case, signal=_strided(case.signal, False)), ref)
    _assert_equal(_call(case, signal=_strided(case.signal, True), chunk=None), ref)
    raw, ss = C.int16_form("lengths")
    want = C.int16_reference("lengths")
    assert want["bad"] == 0 and int(want["n_events"].max()) > 20
    _assert_equal(_call(case, signal=_dev(raw), scale_shift=ss), want)
    _assert_equal(_call(case, signal=_strided(raw, True), scale_shift=ss, chunk=512), want)
    W.check_device_flags()


def test_bad_reads_among_good_ones():
    """NaN in a chunk's interior, inf on a seam, NaN just before one, NaN in the last sample, |q| = 2^23, lengths out of range"""
    case, ref = C.CASES["bad"], C.reference("bad")
    W.check_device_flags()
    got = _call(case)
    _assert_equal(got, ref)
    bad = np.array([name not in C.BAD_GOOD for name in C.BAD_READS])
    assert ref["bad"] == int(bad.sum()) == 7
    assert (got.n_events.cpu().numpy()[bad] == -1).all() and (got.starts.cpu().numpy()[bad] == -1).all()
    assert (got.kind.cpu().numpy()[bad] == -1).all() and not got.sum.cpu().numpy()[bad].any() and not got.sumsq.cpu().numpy()[bad].any()
    with pytest.raises(RuntimeError, match="7 bad read"):
        W.check_device_flags()
    for b in np.flatnonzero(~bad):                                   # the good reads are what they are alone
        alone = C.Case(case.signal[b:b + 1], case.signal_lengths[b:b + 1], case.kw, None)
        one = _call(alone)
        assert all(torch.equal(u[0], v[b]) for u, v in zip(one, got))
    W.check_device_flags()


def test_wrapper_refusals_on_the_device():
    x, n = torch.zeros(2, 300, device=DEV), [300, 300]
    for kw in (dict(windows=(0, 6)), dict(windows=(17, 6)), dict(windows=(3, 17)), dict(windows=(3,)), dict(frac_bits=21), dict(radii=(0, 3)),
               dict(radii=(3, 65)), dict(thresholds=(0.0, 4.0)), dict(thresholds=(4.0, float("nan"))), dict(min_var=-1.0),
               dict(min_var=1e30), dict(thresholds=(1e5, 4.0)), dict(max_event_len=0), dict(max_event_len=65537), dict(max_events=0),
               dict(chunk=128), dict(chunk=300), dict(chunk=32768)):
        with pytest.raises(ValueError, match="detect_events"):
            W.detect_events(x, n, **kw)
    with pytest.raises(ValueError, match="float32 or int16"):
        W.detect_events(x.double(), n)
    got = W.detect_events(x, n, windows=(3, 0), radii=(3, 0), thresholds=(4.0, 0.0))       # the long detector off: its two are ignored
    assert got.n_events.tolist() == [1, 1]
    W.check_device_flags()


def test_repeatable_and_captured():
    case, ref = C.CASES["lengths"], C.reference("lengths")
    a, b = _call(case), _call(case)
    assert all(torch.equal(u, v) for u, v in zip(a, b))              # two runs are bitwise identical
    args = [_dev(case.signal), _dev(case.signal_lengths)]
    kw = dict(case.kw, chunk=512)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        W.detect_events(*args, **kw)                                 # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = W.detect_events(*args, **kw)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(captured, ref)
    assert all(torch.equal(u, v) for u, v in zip(captured, a))
    W.check_device_flags()


def test_composition_raw_reads_to_events_to_mapping_to_alignment():
    """noise-free reads from known loci of a 2000-base reference, a 3-mer table of pairwise distinct levels: detect_events ->
    as_signal -> signal_map gives the true start, end and strand; signal_align of the event means on SignalMapping.labels() gives
    one event per state; kmer_events over the raw samples with detect_events' own starts uses every state.  No bases were supplied"""
    fx = C.composition()
    n = C.COMPOSE_STATES
    signal, lengths = _dev(fx["signal"]), _dev(fx["signal_lengths"])
    ev = W.detect_events(signal, lengths, **fx["kw"])
    assert ev.n_events.tolist() == [n] * 4 and not bool(ev.truncated.any())
    assert np.array_equal(ev.starts.cpu().numpy()[:, 1:n + 1], np.cumsum(fx["dwells"], axis=1))
    assert np.array_equal(ev.length.cpu().numpy()[:, :n], fx["dwells"])
    model = W.signal_model(fx["means"], fx["stdvs"], frac_bits=C.COMPOSE_F)
    reference = W.map_reference(torch.from_numpy(fx["bases"]), model, device=DEV)
    means, counts = ev.as_signal()
    hit = W.signal_map(means, counts, reference)
    assert hit.start.tolist() == fx["start_state"].tolist() and (hit.end - hit.start).tolist() == [n - 1] * 4
    assert hit.strand.tolist() == fx["strand"].tolist() and bool((hit.runner_up > hit.score).all())
    labels, label_lengths = hit.labels()
    al = W.signal_align(means, counts, labels, label_lengths, model, first=0, band=64)
    assert torch.equal(al.score, hit.score)
    assert al.starts[:, :n + 1].tolist() == [list(range(n + 1))] * 4                  # one event per state
    tables = W.kmer_events(signal, lengths, labels, label_lengths, starts=ev.starts[:, :n + 1].contiguous(), k=C.COMPOSE_K, first=0)
    assert tables.read_counts[:, 0].tolist() == [n] * 4 and torch.equal(tables.read_counts[:, 3], lengths)
    assert torch.equal(tables.sum, ev.sum[:, :n]) and torch.equal(tables.sumsq, ev.sumsq[:, :n])
    W.check_device_flags()
