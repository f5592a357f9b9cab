"""GPU: the event tables (csrc/wn_events.hip through wavenet_speech_amd.kmer_events) against the plain-loop reference of
tests/kmer_events_ref.py.  Everything the kernels write is an integer, so every comparison is exact equality; the inputs and their
references are built once in tests/kmer_events_cases.py.  The round trip generate -> segment -> fit is held to six standard errors
of a Gaussian sample: |mean - table| <= 6 sigma / sqrt(n) + 2^-12 (the quantisation step) and |stdv / sigma - 1| <= 6 / sqrt(2 n)."""
import copy

import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import kmer_events_cases as EC
from tests import kmer_events_ref as R
from tests.gpu_signal import assert_kmer_events as _assert_equal, kmer_events as _call
from tests.gpu_util import DEV, dev as _dev, same as _same
from wavenet_speech_amd import synthetic as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("frac_bits", [0, 12])
@pytest.mark.parametrize("kind", EC.KINDS)
@pytest.mark.parametrize("layout", EC.LAYOUTS)
@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_against_the_reference(name, layout, kind, frac_bits):
    case, ref = EC.CASES[name], EC.reference(name, layout, kind, frac_bits)
    more = dict(int16=EC.int16_form(name)) if kind == "i16" else {}
    got = _call(case, layout, kind, frac_bits, strided=frac_bits == 0, **more)       # views by stride in half of the runs
    assert all(t.is_cuda for t in got) and ref["bad"] == 0
    _assert_equal(got, ref)
    W.check_device_flags()


def test_event_levels_on_the_device():
    ref = EC.reference("long_events", "spans", "f32", 12)
    got = _call(EC.CASES["long_events"], "spans", "f32", 12)
    mean, stdv = got.mean.cpu().numpy(), got.stdv.cpu().numpy()
    used = ref["kmer"] >= 0
    n = ref["length"][used].astype(np.float64)
    want = ref["sum"][used] / n / 4096.0
    assert np.isnan(mean[~used]).all() and np.isnan(stdv[~used]).all()
    assert np.abs(mean[used] - want).max() <= 1e-12 * np.abs(want).max()
    var = np.array([(int(s2) * int(m) - int(s1) ** 2) / (int(m) ** 2 * 4096.0 ** 2)
                    for s1, s2, m in zip(ref["sum"][used], ref["sumsq"][used], ref["length"][used])])
    assert np.abs(stdv[used] ** 2 - var).max() <= 1e-9                 # 2^-52 level^2 = 2e-12 at 100 pA, a few operations


@pytest.mark.parametrize("layout", EC.LAYOUTS)
def test_bad_reads_among_good_ones(layout):
    case, ref = EC.bad_batch(), EC.bad_reference(layout)
    seg = EC.bad_segments(layout)[0]
    W.check_device_flags()
    got = _call(case, layout, "f32", 12, seg=seg)
    _assert_equal(got, ref)
    bad = np.array(EC.bad_expected(layout))
    kmer, counts = got.kmer.cpu().numpy(), got.read_counts.cpu().numpy()
    assert (kmer[bad] == -4).all() and (counts[bad] == -1).all() and (counts[~bad, 0] == 16).all()
    for field in (got.start, got.length, got.sum, got.sumsq):
        assert not field.cpu().numpy()[bad].any()
    assert int(got.kmer_stats[:, 0].sum()) == 16 * int((~bad).sum())   # nothing of a bad read in a table
    with pytest.raises(RuntimeError, match="%d bad read" % int(bad.sum())):
        W.check_device_flags()
    # int16: no NaN to meet, but a scale that carries a used sample out of range, a non-finite shift, and a good read between
    raw = np.rint(case.signal[:3, :] * 8.0).astype(np.int16)
    ss = np.array([[0.125, 0.0], [40.0, 0.0], [0.125, np.inf]], dtype=np.float32)
    sub = EC.Case(case.signal[:3], case.signal_lengths[:1].repeat(3), case.labels[:1].repeat(3, 0), case.label_lengths[:1].repeat(3),
                  case.starts[:1].repeat(3, 0), case.gaps[:3], EC.BAD_KW)
    begin, end, events = EC.segments(sub, layout)
    want = R.kmer_events_ref(raw, sub.signal_lengths, sub.labels, sub.label_lengths, begin, end, events, scale_shift=ss, frac_bits=12,
                             **EC.BAD_KW)
    assert want["bad"] == 2 and want["read_counts"][:, 0].tolist() == [16, -1, -1]
    _assert_equal(_call(sub, layout, "i16", 12, int16=(raw, ss)), want)
    with pytest.raises(RuntimeError, match="2 bad read"):
        W.check_device_flags()


def test_round_trip_generate_segment_fit():
    table = S.standin_kmer_table()
    min_count = 100

    def bounds_hold(means, stdvs, counts):
        tm, ts = table[0].double().numpy(), table[1].double().numpy()
        used = counts.numpy() >= min_count
        n = counts.numpy()[used]
        dm = np.abs(means.numpy()[used] - tm[used]) / (6.0 * ts[used] / np.sqrt(n) + 2.0 ** -12)
        ds = np.abs(stdvs.numpy()[used] / ts[used] - 1.0) / (6.0 / np.sqrt(2.0 * n))
        print("k-mers with >= %d samples: %d; worst mean deviation %.3f, worst stdv deviation %.3f of the allowed"
              % (min_count, int(used.sum()), dm.max(), ds.max()))
        assert used.sum() > 300 and dm.max() <= 1.0 and ds.max() <= 1.0
        assert np.isnan(means.numpy()[~used]).all()

    # the same batch size and seed on the CPU first: torch-op reads, the plain-loop reference, the same fit
    g = torch.Generator().manual_seed(5)
    cpu = S.ragged_reads(128, (200, 300), ("uniform", 6, 2), "loader", table, generator=g, device="cpu")
    n_ev = cpu.dwell.shape[1]
    ref = R.kmer_events_ref(cpu.signal[:, 0].numpy(), cpu.signal_lengths.numpy(), cpu.bases.numpy(), cpu.base_lengths.numpy(),
                            cpu.starts[:, :-1].numpy(), cpu.starts[:, 1:].numpy(), np.full(128, n_ev), k=5, first=2, frac_bits=12)
    bounds_hold(*W.fit_kmer_model(ref["kmer_stats"], min_count=min_count))

    g = torch.Generator().manual_seed(5)
    reads = S.ragged_reads(128, (200, 300), ("uniform", 6, 2), "loader", table, generator=g, device="cuda", pad_to=None)
    ev = W.kmer_events(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, starts=reads.starts, first=2)
    W.check_device_flags()
    K = (reads.base_lengths.long() - 8)[:, None]
    live = torch.arange(reads.dwell.shape[1], device=DEV)[None, :] < K
    kmers = S.ragged_kmers(reads.bases, reads.base_lengths, 2)
    assert torch.equal(ev.kmer[live].long(), kmers[live]) and bool((ev.kmer[~live] == -2).all())
    assert torch.equal(ev.length, reads.dwell) and torch.equal(ev.start, reads.starts[:, :-1])
    # sample_kmer names the k-mer (event) of every sample: each event's range holds its own number, and nothing else does
    sk = reads.sample_kmer
    inside = sk >= 0
    first_sample = ev.start.long().gather(1, sk.clamp(min=0).long())
    t = torch.arange(sk.shape[1], device=DEV)[None, :]
    assert bool(((t >= first_sample) & (t < first_sample + ev.length.long().gather(1, sk.clamp(min=0).long())))[inside].all())
    assert torch.equal(inside.sum(1).int(), ev.read_counts[:, 3]) and torch.equal(ev.read_counts[:, 0].long(), K[:, 0])
    means, stdvs, counts = W.fit_kmer_model(ev.kmer_stats, min_count=min_count)
    bounds_hold(means, stdvs, counts)
    assert int(ev.dwell_hist[:, 4:8].sum()) == int(ev.dwell_hist.sum()) == int(K.sum())       # uniform in [4, 8)
    # and the fitted table drives the generator (the k-mers without data from the prior)
    means, stdvs, _ = W.fit_kmer_model(ev.kmer_stats, min_count=min_count, prior=table)
    again = S.ragged_reads(4, (20, 30), ("uniform", 6, 2), "loader", (means, stdvs), generator=g, device="cuda")
    assert bool(torch.isfinite(again.signal).all())


def test_repeatable_accumulating_and_tables_alone():
    first, second = EC.CASES["gaps"], EC.CASES["wave_edges_65_129"]
    a = _call(first, "spans", "f32", 12)
    b = _call(first, "spans", "f32", 12)
    assert _same(a, b)                                               # two runs are bitwise identical
    tables = copy.deepcopy(EC.reference("gaps", "spans", "f32", 12)["tables"])
    begin, end, events = EC.segments(second, "spans")
    want = R.kmer_events_ref(second.signal, second.signal_lengths, second.labels, second.label_lengths, begin, end, events,
                             frac_bits=12, tables=tables, **dict(dict(max_dwell=255), **second.kw))
    got = _call(second, "spans", "f32", 12, into=a)
    assert got.kmer_stats is a.kmer_stats and got.dwell_hist is a.dwell_hist
    _assert_equal(got, want)                                         # the reference of the two batches one after the other
    assert int(got.kmer_stats[:, 0].sum()) > int(b.kmer_stats[:, 0].sum()) > 0
    alone = _call(first, "spans", "f32", 12, want_events=False)
    _assert_equal(alone, EC.reference("gaps", "spans", "f32", 12), events=False)
    assert torch.equal(alone.kmer_stats, b.kmer_stats) and torch.equal(alone.dwell_hist, b.dwell_hist)
    with pytest.raises(ValueError, match="into"):
        _call(second, "spans", "f32", 0, into=b)                     # other frac_bits: the tables do not add up
    with pytest.raises(ValueError, match="exactly one"):
        W.kmer_events(_dev(first.signal), _dev(first.signal_lengths), _dev(first.labels), _dev(first.label_lengths))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.kmer_events(torch.from_numpy(first.signal), first.signal_lengths, first.labels, first.label_lengths, starts=first.starts)
    W.check_device_flags()


def test_captured_call_replays_the_same_tables():
    case = EC.CASES["wave_edges_65_129"]
    args = [_dev(case.signal), _dev(case.signal_lengths), _dev(case.labels), _dev(case.label_lengths)]
    starts = _dev(case.starts)
    eager = W.kmer_events(*args, starts=starts, **case.kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        W.kmer_events(*args, starts=starts, **case.kw)               # warm the allocator on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = W.kmer_events(*args, starts=starts, **case.kw)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(captured, eager)
    _assert_equal(captured, EC.reference("wave_edges_65_129", "starts", "f32", 12))
    W.check_device_flags()
