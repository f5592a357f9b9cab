"""GPU: kmer_events, signal_align and signal_map (csrc/wn_events.hip, wn_sigalign.hip, wn_sigmap.hip and what they share,
csrc/wn_signal_dev.h) at their numeric limits, against tests/kmer_events_ref.py, tests/signal_align_ref.py and
tests/signal_map_ref.py.  Everything the kernels write is an integer and every comparison is exact equality.  The inputs, their
references and the vectorised table reference are built once in tests/signal_limits_cases.py; tests/test_signal_limits_ref.py
asserts on the CPU that they reach what each test below names."""
import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from tests import signal_align_ref as AR
from tests import signal_limits_cases as C
from tests import signal_map_ref as MR
from tests.gpu_signal import assert_kmer_events as _assert_events_equal, assert_signal_alignment as _assert_align_equal
from tests.gpu_signal import assert_signal_mapping as _assert_map_equal
from tests.gpu_util import DEV, dev as _dev, no_stale_flags  # noqa: F401

pytestmark = pytest.mark.gpu


I64_MIN = np.iinfo(np.int64).min


def _model(table, weight_shift, frac_bits):
    return W.SignalModel(torch.from_numpy(np.asarray(table, dtype=np.int64)), weight_shift, frac_bits, C.COST_BITS)


def _events(case, k=1, first=0, **more):
    return W.kmer_events(_dev(case.signal), _dev(case.signal_lengths), _dev(case.labels), _dev(case.label_lengths), starts=_dev(case.starts),
                         k=k, first=first, **more)


def _expect_bad(n):
    if n == 0:
        W.check_device_flags()
    else:
        with pytest.raises(RuntimeError, match="%d bad read" % n):
            W.check_device_flags()


# ---- 1. the sample cost, read straight off the device
@pytest.mark.parametrize("S", C.GRID_SHIFTS)
def test_sample_cost_over_the_grid(S):
    """64 model rows over level in {+-(2^23 - 1), +-1, 0, mid}, weight in {1, 2, 2^16, 2^30, 2^31 - 1, odd}, offset in {+-(2^30 - 1), 0}
    against 40 samples from 0 to +-(2^23 - 1), at F in {0, 20} and max_cost in {1, 12345, 2^31 - 1}: d up to 2^24 - 2, products of 79
    bits, clamped and un-clamped at every S.  signal_map of one-sample reads shows the whole matrix as end_cost (and score, end,
    start, the block table); signal_align with T = N = 1 shows one cell per read as its score"""
    codes, _ = MR.prepare(C.grid_reference(), C.grid_model(), C.GRID_K)
    open_states = np.flatnonzero(codes >= 0)
    ones = torch.ones(40, dtype=torch.int32, device=DEV)
    W.check_device_flags()
    for F in C.GRID_FRAC:
        model = _model(C.grid_model(), S, F)
        reference = W.map_reference(torch.from_numpy(C.grid_reference()), model, both_strands=False, device=DEV)
        assert reference.n_states == 75
        signal = _dev(C.grid_signal(F))
        reads, labels = (_dev(a) for a in C.grid_align_inputs(F))
        n = reads.shape[0]
        lengths, label_lengths = torch.ones(n, dtype=torch.int32, device=DEV), torch.full((n,), C.GRID_K, dtype=torch.int32, device=DEV)
        for max_cost in C.GRID_MAX_COSTS:
            costs = np.array(C.grid_costs(S, max_cost), dtype=np.int64)                  # [40, 64], from sample_cost
            got = W.signal_map(signal, ones, reference, max_cost=max_cost, want_end_cost=True)
            assert np.array_equal(got.end_cost.cpu().numpy()[:, open_states], costs[:, codes[open_states]]), (F, max_cost)
            _assert_map_equal(got, C.grid_map_reference(F, S, max_cost))
            al = W.signal_align(reads, lengths, labels, label_lengths, model, first=0, band=64, max_cost=max_cost, want_states=True)
            assert np.array_equal(al.score.cpu().numpy(), costs.reshape(-1)), (F, max_cost)
            assert al.starts.cpu().tolist() == [[0, 1]] * n and not bool(al.band_hits.any())
            assert al.states.cpu().tolist() == [[0, -1]] * n
    W.check_device_flags()


# ---- 2. quantisation, read through one-sample events
def _quant_cases():
    return [C.quant_f32_case(F) for F in C.QUANT_FRAC] + [C.quant_i16_case()]


@pytest.mark.parametrize("index", range(5), ids=["f32_F%d" % F for F in C.QUANT_FRAC] + ["i16_F12"])
def test_quantisation_edges_seen_alike_by_the_three_tools(index):
    """float32 at F in {0, 1, 12, 20}: ties both ways (near 0 and at 23 and 24 significant bits), -0.0, a denormal, +-(2^23 - 1); the
    first value out of range on each sign and the tie that rounds onto it, each in a read of its own among good ones.  int16 with
    scale_shift at F = 12: raw values up to +-32768, scales 0.5 and float32(0.1) with shifts at which float32 arithmetic would round
    the other way, a pair that lands on +-(2^23 - 1), and one step beyond by the shift and by the scale.  kmer_events with
    one-sample events returns q as its sum; the same samples as one-sample reads cost (q - level)^2 in signal_map and signal_align,
    under a model that holds a row at level 0 and one at every expected q and its successor"""
    cases = _quant_cases()
    case = cases[index]
    ss = None if case.scale_shift is None else _dev(case.scale_shift)
    want_q = C.quant_expected_q(case)
    B, n = case.signal.shape
    W.check_device_flags()
    ev = _events(case, scale_shift=ss, frac_bits=case.frac_bits)
    _assert_events_equal(ev, C.quant_events_reference(case))
    _expect_bad(3)
    q_dev = ev.sum.cpu().numpy()
    bad_read = np.array([None in row for row in want_q])
    assert q_dev[~bad_read].tolist() == [row for row in want_q if None not in row]

    table = C.quant_model(cases)
    levels = table[:, 0].tolist()
    model = _model(table, 16, case.frac_bits)
    ref_bases = np.array(C.de_bruijn(C.QUANT_K), dtype=np.int32)
    codes, _ = MR.prepare(ref_bases, table, C.QUANT_K)
    state_of = np.argsort(codes)                                     # the state that holds k-mer c
    signal, ss_rows = C.quant_samples_as_reads(case)
    costs = C.quant_costs(case, table)
    bad = np.array([c is None for c in costs])
    want = np.array([[I64_MIN] * 64 if c is None else c for c in costs], dtype=np.int64)
    reference = W.map_reference(torch.from_numpy(ref_bases), model, both_strands=False, device=DEV)
    ones = torch.ones(B * n, dtype=torch.int32, device=DEV)
    got = W.signal_map(_dev(signal), ones, reference, scale_shift=None if ss_rows is None else _dev(ss_rows), want_end_cost=True)
    end_cost = got.end_cost.cpu().numpy()
    assert np.array_equal(end_cost, want[:, codes])
    _assert_map_equal(got, MR.signal_map_ref(signal, np.ones(B * n, dtype=np.int32), ref_bases, table, C.QUANT_K, frac_bits=case.frac_bits,
                                             weight_shift=16, scale_shift=ss_rows))
    assert (got.score.cpu().numpy()[bad] == I64_MIN).all() and int(bad.sum()) == 3
    _expect_bad(3)

    # signal_align: every sample twice, in the k-mer whose level is its expected q and in the k-mer of level 0
    own = [0 if c is None else levels.index(q) for c, q in zip(costs, [q for row in want_q for q in row])]
    labels = np.array([C.kmer_labels(c, C.QUANT_K) for c in own] + [C.kmer_labels(0, C.QUANT_K)] * (B * n), dtype=np.int32)
    twice = np.concatenate([signal, signal])
    al = W.signal_align(_dev(twice), torch.ones(2 * B * n, dtype=torch.int32, device=DEV), _dev(labels),
                        torch.full((2 * B * n,), C.QUANT_K, dtype=torch.int32, device=DEV), model, first=0, band=64,
                        scale_shift=None if ss_rows is None else _dev(np.concatenate([ss_rows, ss_rows])))
    score = al.score.cpu().numpy()
    assert np.array_equal(score, np.concatenate([want[np.arange(B * n), own], want[:, 0]]))
    assert AR.BAD_READ == I64_MIN and (score[:B * n][bad] == I64_MIN).all()
    _expect_bad(6)

    # and among themselves: the q that kmer_events returned costs 0 in its own row and min(q^2, 2^31 - 1) in row 0, in both tools
    flat_q = q_dev.reshape(-1)
    good = np.flatnonzero(~np.repeat(bad_read, n))
    assert not bad[good].any()
    for i in good.tolist():
        q = int(flat_q[i])
        assert end_cost[i, state_of[levels.index(q)]] == 0 == score[i] and end_cost[i, state_of[0]] == min(q * q, C.COST_MAX) == score[B * n + i]
    W.check_device_flags()


# ---- 3. event sums at their largest and negative
def test_event_sums_at_their_largest_and_negative():
    """every sample -(2^23 - 1) in one read and +(2^23 - 1) in the other, events of 65536, 65536, 33, 32 and 1 samples: sums of
    -+2^39 and 2^62 per event through the wave path, across the 32 / 33 seam and in one lane; a negative sum added in two's complement
    in LDS and in global memory; limb sums past 32 bits; the clamp column; a second call into the same tables; the fit"""
    case = C.big_case()
    W.check_device_flags()
    ref = C.big_reference()
    got = _events(case, max_dwell=255, **C.BIG_KW)
    _assert_events_equal(got, ref)
    assert int(got.sum[0, 0]) == -C.Q_MAX * 65536 and int(got.sumsq[1, 1]) == C.Q_MAX ** 2 * 65536
    assert int(got.dwell_hist[C.BIG_BASE - 1, 255]) == 4
    again = _events(case, max_dwell=255, into=got, **C.BIG_KW)
    assert again.kmer_stats is got.kmer_stats
    _assert_events_equal(again, C.big_reference(twice=True))
    for read, sign in ((0, -1), (1, 1)):
        alone_ref = C.big_reference(reads=(read,), max_dwell=65536)
        alone = _events(C.big_rows([read]), max_dwell=65536, **C.BIG_KW)
        _assert_events_equal(alone, alone_ref)
        assert int(alone.dwell_hist[C.BIG_BASE - 1, 65536]) == 2
        _, samples, s1, lo, hi = [int(v) for v in alone.kmer_stats[C.BIG_BASE - 1].cpu().tolist()]
        assert s1 == sign * C.Q_MAX * 131138 and (hi << 32) + lo == C.Q_MAX ** 2 * 131138
        means, stdvs, counts = W.fit_kmer_model(alone.kmer_stats, frac_bits=0, min_count=1)
        assert float(means[C.BIG_BASE - 1]) == s1 / samples and float(stdvs[C.BIG_BASE - 1]) == 0.0 and float(counts[C.BIG_BASE - 1]) == samples
        tables_only = _events(C.big_rows([read]), max_dwell=65536, want_events=False, **C.BIG_KW)
        _assert_events_equal(tables_only, alone_ref, events=False)
    W.check_device_flags()


# ---- 4. the table kernel across workgroups
@pytest.mark.parametrize("name,k", [("three", 2), ("three", 6), ("cap", 1), ("cap", 6)])
def test_tables_across_workgroups(name, k):
    """three: 37 x 300 events are 3 workgroups of 3840 rows, the seams inside reads 12 (bad: a NaN) and 25, read 30 bad by its
    length; k = 2 adds into 16 LDS rows under contention, k = 6 straight into global memory.  cap: 2050 x 513 one-sample events are
    more than 256 x 4096 rows: 256 workgroups of 4352 rows, 242..255 with nothing to do, bad reads on the seams of workgroups 1, 100
    and 241 and at the end.  Every output, with and without the per-event rows, against the vectorised reference"""
    case, ref = C.table_case(name), C.table_reference(name, k)
    B, N = case.starts.shape[0], case.starts.shape[1] - 1
    assert C.table_grid(B * N) == {"three": (3, 3840), "cap": (256, 4352)}[name]
    W.check_device_flags()
    got = _events(case, k=k, first=C.TABLE_WINDOWS[k])
    _assert_events_equal(got, ref)
    _expect_bad(len(case.bad_reads))
    tables_only = _events(case, k=k, first=C.TABLE_WINDOWS[k], want_events=False)
    _assert_events_equal(tables_only, ref, events=False)
    _expect_bad(len(case.bad_reads))
    assert ref["bad"] == len(case.bad_reads)


# ---- 5. long paths
@pytest.mark.parametrize("which", ["costly", "cheap"])
def test_signal_map_at_its_longest_read(which):
    """L = T = max_signal = 4096 (the whole 64 KiB of dynamic LDS and the longest boundary column), reads of 4095 and 1 samples
    beside it, 5200 states with two walls, strips of 64 and 2048 states and the automatic one.  costly: nearly every cell costs
    2^31 - 1 + 2^30 - 1, a total near 2^43.6; cheap: nearly every cell costs -(2^30 - 1), a total near -2^42, not the bad-read
    sentinel"""
    case, ref = C.map_long_case(which), C.map_long_reference(which)
    model = _model(case.model, case.kw["weight_shift"], case.kw["frac_bits"])
    reference = W.map_reference(torch.from_numpy(case.ref), model, both_strands=False, device=DEV)
    assert reference.n_states == C.MAP_M and case.signal.shape[1] == 4096
    signal, lengths = _dev(case.signal), _dev(case.signal_lengths)
    W.check_device_flags()
    runs = [W.signal_map(signal, lengths, reference, max_cost=case.kw["max_cost"], strip=strip, want_end_cost=True) for strip in C.MAP_STRIPS]
    for got in runs:
        _assert_map_equal(got, ref)
        assert all(torch.equal(u, v) for u, v in zip(got, runs[0]))
    assert (runs[0].score.cpu().numpy() != I64_MIN).all() and bool(runs[0].mapped.all())
    W.check_device_flags()


@pytest.mark.parametrize("band", sorted(C.DIAGONAL))
@pytest.mark.parametrize("which", ["costly", "cheap"])
def test_signal_align_on_the_forced_diagonal(which, band):
    """N == T in {65, 320, 321, 577} at band 64 and N == T = 600 at band 512: the band rises on every step and the only path is the
    diagonal, so the score is the plain sum of the cells along it; T = N + 1 beside each; the two models of extreme cost"""
    case, ref = C.diagonal_case(which, band), C.diagonal_reference(which, band)
    model = _model(case.model, case.kw["weight_shift"], case.kw["frac_bits"])
    W.check_device_flags()
    got = W.signal_align(_dev(case.signal), _dev(case.signal_lengths), _dev(case.labels), _dev(case.label_lengths), model, first=0,
                         band=band, max_cost=case.kw["max_cost"], want_states=True)
    _assert_align_equal(got, ref)
    score = got.score.cpu().tolist()
    for b, (T, N) in enumerate(C.DIAGONAL[band]):
        if T == N:
            assert score[b] == C.diagonal_sum(case, b) and got.states[b, :T].cpu().tolist() == list(range(N))
    W.check_device_flags()
