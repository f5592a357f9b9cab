"""GPU: the ragged read generator (csrc/wn_reads.hip: wn_reads_plan, wn_reads_signal) against the reference's fixture
(tests/golden/ragged_00.npz), against the torch form of the same arithmetic (ragged_reads on device="cpu") on given bases, dwell
and noise, and -- for the random stages -- against the exact distributions (tests/dwell_stats.py, validated on the CPU by
tests/test_ragged_reads.py).  All shapes are tiny.

Tolerances: integers (lengths, starts, the k-mer of every sample) are exact.  The signal is (float)(mean + stdv * z) with the sum
in float64: a fused multiply-add may move the float64 sum by one of ITS ulps before the single rounding to float32, so the
float32 result may differ from the two-rounding form by at most one float32 ulp (and almost never does)."""
import pytest
import torch

import wavenet_speech_amd as W
from wavenet_speech_amd import synthetic as S
from tests import dwell_stats as D
from tests.cpu_util import gold, ragged_table as _table  # noqa: F401
from tests.gpu_labels import plan_given as _plan_given
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


def _ulps(a, b):
    """largest distance in float32 ulps between two float32 tensors of one sign"""
    return int((a.cpu().contiguous().view(torch.int32).long() - b.cpu().contiguous().view(torch.int32).long()).abs().max())


@pytest.mark.parametrize("case", ["case0", "case1", "case2"])
def test_fixture_read_through_the_c_abi(gold, case):
    g = lambda k: torch.from_numpy(gold[case + "." + k])
    window = int(gold[case + ".window"])
    bases, dwell, noise = g("bases")[None], g("dwell")[None], g("noise")[None]
    n, K, L = bases.shape[1], dwell.shape[1], noise.shape[1]
    plan = _plan_given(bases, torch.tensor([n]), dwell, window)
    signal, sample_kmer, clipped, bad = S.hip_reads_signal(plan, L, _table(gold), 0, noise.to(DEV).contiguous())
    assert int(plan["bad"]) == 0 and int(bad) == 0 and int(plan["clamped"]) == 0
    assert int(plan["base_lengths"][0]) == n and int(plan["signal_lengths"][0]) == L and int(clipped[0]) == L
    assert torch.equal(plan["bases"][0, :n].cpu().long(), bases[0]) and int(plan["bases"][0, n]) == 0
    assert torch.equal(plan["dwell"][0, :K].cpu().long(), dwell[0]) and not plan["dwell"][0, K:].any()
    want_starts = torch.cat([torch.zeros(1, dtype=torch.long), dwell[0].cumsum(0)])
    assert torch.equal(plan["starts"][0, :K + 1].cpu().long(), want_starts) and bool((plan["starts"][0, K:] == L).all())
    kmers = S.ragged_kmers(bases, torch.tensor([n]), window)[0]
    assert torch.equal(kmers, g("kmers"))
    assert torch.equal(kmers[sample_kmer[0].cpu().long()], g("kmer_seq"))
    ulps = _ulps(signal[0], g("signal_f32"))
    print("%s: %d samples, worst distance to the reference's float32 signal %d ulp" % (case, L, ulps))
    assert ulps <= 1


def test_fixture_batch_through_ragged_reads(gold):
    g = lambda k: torch.from_numpy(gold["batch." + k])
    r = W.ragged_reads(3, window="loader", table=_table(gold), bases=g("bases"), base_lengths=g("lengths"), dwell_values=g("dwell"),
                       noise=g("noise"), device=DEV)
    want = g("signal_f32")
    assert r.signal.shape == (3, 1, want.shape[1]) and r.signal.is_cuda
    assert torch.equal(r.signal_lengths.cpu().long(), g("signal_lengths"))
    assert torch.equal(r.targets.cpu(), g("seq")) and torch.equal(r.base_lengths.cpu(), g("lengths"))
    assert _ulps(r.signal[:, 0], want) <= 1
    for b in range(3):
        n = int(r.signal_lengths[b])
        assert not r.signal[b, 0, n:].any() and bool((r.sample_kmer[b, n:] == -1).all())


SCAN_K = [1, 63, 64, 65, 255, 256, 257, 1025, 5000]


def test_scan_edges_match_cumsum():
    gen = torch.Generator().manual_seed(21)
    kmax = max(SCAN_K)
    dwell = torch.randint(1, 12, (len(SCAN_K), kmax), generator=gen)
    lengths = torch.tensor(SCAN_K) + 4                                  # window 0: K = n - 4
    plan = _plan_given(None, lengths, dwell, 0)
    assert int(plan["bad"]) == 0
    for b, K in enumerate(SCAN_K):
        want = torch.cat([torch.zeros(1, dtype=torch.long), dwell[b, :K].cumsum(0)])
        assert torch.equal(plan["starts"][b, :K + 1].cpu().long(), want), K
        assert int(plan["signal_lengths"][b]) == int(want[-1])
        assert bool((plan["starts"][b, K:] == int(want[-1])).all()) and not plan["dwell"][b, K:].any()
        assert torch.equal(plan["dwell"][b, :K].cpu().long(), dwell[b, :K])
        n = K + 4
        assert bool(((plan["bases"][b, :n] >= 1) & (plan["bases"][b, :n] <= 4)).all()) and not plan["bases"][b, n:].any()


def _compose(total, parts, gen):
    """`parts` positive integers that sum to `total`"""
    cuts = torch.randperm(total - 1, generator=gen)[:parts - 1].sort().values + 1
    edges = torch.cat([torch.zeros(1, dtype=torch.long), cuts, torch.tensor([total])])
    return (edges[1:] - edges[:-1]).tolist()


def _tile_cases():
    gen = torch.Generator().manual_seed(31)
    rows = [[1], _compose(255, 40, gen), _compose(256, 40, gen), _compose(257, 41, gen), _compose(513, 90, gen),
            [1] * 600,                                     # every sample its own k-mer
            [2] + [1] * 599,                               # the same, one sample out of phase with the tiles
            [3, 1000, 2, 1, 1, 300, 1],                    # a k-mer that spans several tiles
            [700]]                                         # K = 1, longer than two tiles
    K = max(len(r) for r in rows)
    dwell = torch.zeros(len(rows), K, dtype=torch.long)
    for b, r in enumerate(rows):
        dwell[b, :len(r)] = torch.tensor(r)
    lengths = torch.tensor([len(r) for r in rows]) + 8     # window 2
    bases = torch.randint(1, 5, (len(rows), int(lengths.max())), generator=gen)
    return bases, lengths, dwell, gen


def test_tile_edges_match_the_torch_form():
    bases, lengths, dwell, gen = _tile_cases()
    lmax = int(dwell.sum(1).max())
    assert lmax == 1308 and lmax % 256 != 0
    table = S.standin_kmer_table()
    for ld in (None, lmax + 3, 1536):                                   # the longest read; not a multiple of 256; a multiple
        noise = torch.randn(bases.shape[0], ld or lmax, generator=gen, dtype=torch.float64)
        kw = dict(window="loader", table=table, bases=bases, base_lengths=lengths, dwell_values=dwell, noise=noise, pad_to=ld)
        want = S.ragged_reads(bases.shape[0], device="cpu", **kw)
        got = S.ragged_reads(bases.shape[0], device=DEV, **kw)
        assert got.signal.shape == want.signal.shape == (bases.shape[0], 1, ld or lmax)
        for name in ("signal_lengths", "bases", "base_lengths", "dwell", "starts", "sample_kmer"):
            assert torch.equal(getattr(got, name).cpu(), getattr(want, name)), (ld, name)
        inside = want.sample_kmer >= 0
        assert not got.signal[:, 0].cpu()[~inside].any()
        # one sign inside the reads (picoamps are positive); padding is exactly zero on both sides
        assert _ulps(got.signal[:, 0].cpu() * inside, want.signal[:, 0] * inside) <= 1, ld
        if ld is None:
            assert torch.equal(got.targets.cpu(), want.targets)
    W.check_device_flags()


def test_every_output_element_is_written():
    bases, lengths, dwell, gen = _tile_cases()
    plan = _plan_given(bases, lengths, dwell, 2)
    B, ld = bases.shape[0], 1308 + 77
    for fill_signal, fill_kmer in ((float("nan"), 0x7f7f7f7f), (-1.0, 0)):
        signal = torch.full((B, ld), fill_signal, dtype=torch.float32, device=DEV)
        sample_kmer = torch.full((B, ld), fill_kmer, dtype=torch.int32, device=DEV)
        S.hip_reads_signal(plan, ld, S.standin_kmer_table(), 5, None, signal, sample_kmer)
        for b in range(B):
            n, K = int(plan["signal_lengths"][b]), int(lengths[b]) - 8
            assert not signal[b, n:].any() and bool((sample_kmer[b, n:] == -1).all())        # exactly 0.0 and -1, to the end
            assert bool((signal[b, :n] > 0).all()) and bool(((sample_kmer[b, :n] >= 0) & (sample_kmer[b, :n] < K)).all())
            assert torch.equal(torch.bincount(sample_kmer[b, :n].long(), minlength=K).cpu(), dwell[b, :K])


def test_poisoned_reads_and_overflow_are_flagged_not_indexed():
    gen = torch.Generator().manual_seed(41)
    bases = torch.randint(1, 5, (6, 40), generator=gen)
    dwell = torch.randint(1, 9, (6, 32), generator=gen)
    lengths = torch.tensor([40, 8, 1 << 30, -5, 40, 40])                # 8 < 9, far too long, negative
    dwell[4, 7] = 0                                                     # a dwell below 1
    bases[5, 11] = 9                                                    # not a nucleotide
    plan = _plan_given(bases, lengths, dwell, 2)
    assert int(plan["bad"]) == 5
    assert plan["base_lengths"].tolist() == [40, 0, 0, 0, 0, 0] and plan["signal_lengths"].tolist()[1:] == [0] * 5
    assert int(plan["signal_lengths"][0]) == int(dwell[0].sum())
    assert not plan["bases"][1:].any() and not plan["dwell"][1:].any() and not plan["starts"][1:].any()
    signal, sample_kmer, clipped, bad = S.hip_reads_signal(plan, 300, S.standin_kmer_table(), 5)
    assert int(bad) == 0 and clipped.tolist() == plan["signal_lengths"].tolist()
    assert not signal[1:].any() and bool((sample_kmer[1:] == -1).all()) and bool((signal[0, :int(clipped[0])] > 0).all())
    # a row shorter than the read: truncated, the clipped length reported, counted
    signal, sample_kmer, clipped, bad = S.hip_reads_signal(plan, 100, S.standin_kmer_table(), 5)
    assert int(bad) == 1 and clipped.tolist() == [100, 0, 0, 0, 0, 0]
    assert bool((signal[0] > 0).all()) and bool((sample_kmer[0] >= 0).all()) and int(sample_kmer[0].max()) < 32
    # the clamp: values above max_dwell are cut to it and counted
    plan = _plan_given(bases[:1], lengths[:1], dwell[:1], 2, max_dwell=5)
    assert int(plan["clamped"]) == int((dwell[0] > 5).sum()) > 0
    assert torch.equal(plan["dwell"][0, :32].cpu().long(), dwell[0].clamp(max=5))
    # the Python surface: at once without pad_to, through the flag watch with it
    with pytest.raises(RuntimeError, match="ragged_reads"):
        W.ragged_reads(6, bases=bases, base_lengths=lengths, dwell_values=dwell, device=DEV)
    W.ragged_reads(4, (20, 30), ("fixed", 3), pad_to=63, device=DEV)    # 12 to 21 k-mers of 3 samples: 36 to 63
    W.check_device_flags()
    W.ragged_reads(4, (20, 30), ("fixed", 3), pad_to=30, device=DEV)
    with pytest.raises(RuntimeError, match="pad_to"):
        W.check_device_flags()


def _dwell_draws(dwell, n_draws, seed):
    """at least n_draws dwell times of the device's stream: 49 loader reads of 4100 bases (4092 k-mers each)"""
    plan = S.hip_reads_plan(49, 4100, 4101, 2, dwell, S.default_max_dwell(dwell), seed, DEV)
    assert int(plan["bad"]) == 0 and bool((plan["base_lengths"] == 4100).all())
    assert int(plan["clamped"]) == 0                                    # the default clamp has an upper tail below 1e-12
    return plan["dwell"][:, :4092].flatten()[:n_draws]


def test_random_lengths_and_uniform_dwell():
    r = W.ragged_reads(2000, (20, 30), ("uniform", 6, 2), generator=torch.Generator().manual_seed(2), device=DEV, pad_to=160)
    W.check_device_flags()
    assert sorted(set(r.base_lengths.tolist())) == list(range(20, 30))  # exactly [lo, hi)
    counts = torch.bincount(r.base_lengths.long().cpu(), minlength=30)[20:].double() / 2000
    assert float((counts - 0.1).abs().max()) < 0.04                     # 6 sigma of a binomial(2000, 0.1) share is 0.040
    live = r.dwell[r.dwell > 0]
    assert int(live.min()) == 4 and int(live.max()) == 7
    assert torch.equal((r.dwell > 0).sum(1).int(), r.base_lengths - 8)
    nt = torch.bincount(r.bases.flatten().long().cpu(), minlength=5)[1:].double()
    assert float((nt / nt.sum() - 0.25).abs().max()) < 0.01
    draws = _dwell_draws(("uniform", 6, 2), 200000, 77)
    stat, dof, outside = D.chi_square(draws, D.uniform_pmf(6, 2))
    print("uniform (6, 2): chi2 %.1f, dof %d, bound %.1f, outside %d" % (stat, dof, D.chi_square_quantile(dof), outside))
    assert D.accepts(draws, D.uniform_pmf(6, 2))
    assert not D.accepts(draws, D.uniform_pmf(6, 3))
    lo1 = _dwell_draws(("uniform", 1, 2), 50000, 78)                   # the interval clipped at 1: [1, 3)
    assert D.accepts(lo1, D.uniform_pmf(1, 2)) and int(lo1.min()) == 1 and int(lo1.max()) == 2


@pytest.mark.parametrize("shape", [2.461964, 0.5])
def test_gamma_dwell_matches_the_exact_pmf(shape):
    dwell = ("gamma", shape, 587.2858, 4000.0)
    draws = _dwell_draws(dwell, 200000, 79)
    pmf = D.gamma_floor_pmf(shape, 587.2858, 4000.0)
    stat, dof, outside = D.chi_square(draws, pmf)
    print("gamma shape %g: chi2 %.1f, dof %d, bound %.1f, outside %d, mean %.3f" % (shape, stat, dof, D.chi_square_quantile(dof), outside,
                                                                                  float(draws.double().mean())))
    assert int(draws.min()) >= 1
    assert D.accepts(draws, pmf)
    assert not D.accepts(draws, D.gamma_floor_pmf(shape * 1.05, 587.2858, 4000.0))


def test_noise_moments_and_reproducibility():
    means, stdvs = S.standin_kmer_table()
    kw = dict(lengths=(4000, 4010), dwell=("uniform", 6, 2), window="loader", table=(means, stdvs), device=DEV)
    r = W.ragged_reads(10, generator=torch.Generator().manual_seed(3), **kw)
    kmers = S.ragged_kmers(r.bases, r.base_lengths, 2)
    md, sd = means.double().to(DEV), stdvs.double().to(DEV)
    zs = []
    for b in range(10):
        n = int(r.signal_lengths[b])
        k = kmers[b][r.sample_kmer[b, :n].long()]
        zs.append((r.signal[b, 0, :n].double() - md[k]) / sd[k])
    z = torch.cat(zs)
    assert z.numel() > 200000
    # the bars of test_hip_generator_random_stages_and_full_size (tests/test_synthetic.py), at the same sample count
    assert abs(float(z.mean())) < 0.01 and abs(float(z.std()) - 1.0) < 0.01
    assert abs(float((z ** 3).mean())) < 0.03 and abs(float((z ** 4).mean()) - 3.0) < 0.08
    assert abs(float((z[1:] * z[:-1]).mean())) < 0.01
    # the same seed gives the same bits, another seed does not
    small = dict(kw, lengths=(20, 30), pad_to=160)
    for dwell in (("uniform", 6, 2), ("gamma", 2.461964, 587.2858, 800.0)):
        small["dwell"] = dwell
        a = W.ragged_reads(7, generator=torch.Generator().manual_seed(9), **small)
        b = W.ragged_reads(7, generator=torch.Generator().manual_seed(9), **small)
        c = W.ragged_reads(7, generator=torch.Generator().manual_seed(10), **small)
        for name in ("signal", "signal_lengths", "bases", "base_lengths", "dwell", "starts", "sample_kmer"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert not torch.equal(a.signal, c.signal) and not torch.equal(a.bases, c.bases) and not torch.equal(a.dwell, c.dwell)
        # a read depends on (seed, b) only: read b of a batch of 2 is read b of a batch of 7
        two = W.ragged_reads(2, generator=torch.Generator().manual_seed(9), **small)
        for name in ("signal", "signal_lengths", "bases", "base_lengths", "dwell", "starts", "sample_kmer"):
            assert torch.equal(getattr(two, name), getattr(a, name)[:2]), name
    W.check_device_flags()


def test_greedy_decode_recovers_bases_and_starts():
    for window, dwell in (("loader", ("uniform", 6, 2)), ("generator", ("gamma", 2.461964, 587.2858, 4000.0))):
        r = W.ragged_reads(5, (20, 30), dwell, window, generator=torch.Generator().manual_seed(13), device=DEV)
        B, L = r.signal.shape[0], r.signal.shape[2]
        c = S.WINDOWS[window] + 2                                       # the centre base of k-mer p is bases[p + c]
        K = r.base_lengths.long() - 4 - 2 * S.WINDOWS[window]
        logits = torch.zeros(B, 5, L, device=DEV)
        logits[:, 0] = 1.0                                              # blank everywhere ...
        for b in range(B):
            k = int(K[b])
            first = r.starts[b, :k].long()
            logits[b, 0, first] = 0.0
            logits[b, r.bases[b, c:c + k].long(), first] = 5.0          # ... but the first sample of every k-mer span
        labels, lengths, frames = W.ctc_greedy_decode(logits, input_lengths=r.signal_lengths)
        for b in range(B):
            k = int(K[b])
            if dwell[0] == "uniform":                                   # every dwell >= 4: a blank between any two labels
                assert int(lengths[b]) == k
                assert torch.equal(labels[b, :k], r.bases[b, c:c + k]) and torch.equal(frames[b, :k], r.starts[b, :k])
            else:                                                       # a dwell of 1 merges two equal neighbours, as CTC does
                keep = torch.ones(k, dtype=torch.bool, device=DEV)
                keep[1:] = ~((r.dwell[b, :k - 1] == 1) & (r.bases[b, c + 1:c + k] == r.bases[b, c:c + k - 1]))
                assert int(lengths[b]) == int(keep.sum())
                assert torch.equal(labels[b, :int(lengths[b])], r.bases[b, c:c + k][keep])
                assert torch.equal(frames[b, :int(lengths[b])], r.starts[b, :k][keep])


def test_rawctcnet_trains_on_ragged_reads():
    from wavenet_speech_amd import training as T
    torch.manual_seed(0)
    net = W.RawCTCNet(16, 3, 5, [(16, 16, 2, d) for d in (1, 2)], 16, softmax=False).to(DEV)
    ld = W.RawGaussianModelLoader(10, 1, 10, None, batch_size=4, upsampling=6, random_upsample=True, lengths=(20, 30))
    ld.cuda()
    ld.generator = torch.Generator().manual_seed(5)
    reads = ld.fetch_reads()
    assert reads.signal.is_cuda and ld.counter == 1
    signal = (reads.signal - 90.0) / 20.0                               # picoamps around 90 +- 30
    out = net(signal)
    assert out.shape[:2] == (4, 5) and out.shape[2] >= int(reads.signal_lengths.max())
    loss = T.ctc_total(out, reads.bases.long(), reads.base_lengths.long(), input_lengths=reads.signal_lengths.long())
    loss.backward()
    W.check_device_flags()
    assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
    # a parameter whose output nothing reads (the residual path of the last block) has no gradient at all; every gradient
    # that exists is finite, and both ends of the network have one that is not zero
    named = dict(net.named_parameters())
    missing = sorted(k for k, p in named.items() if p.grad is None)
    print("parameters without a gradient:", missing)
    assert all(bool(torch.isfinite(p.grad).all()) for p in named.values() if p.grad is not None)
    for k in ("feature_layer.0.weight", "output_block.3.weight", "convolutions.0.conv1x1_residual.weight"):
        assert named[k].grad is not None and float(named[k].grad.abs().max()) > 0, k
    assert len(missing) < len(named) // 2
    sig, seq, lengths = ld.fetch()
    assert sig.is_cuda and sig.dim() == 2 and seq.dtype == torch.int32 and int(seq.numel()) == int(lengths.sum())
