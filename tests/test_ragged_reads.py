"""CPU: the ragged read generator as torch ops (wavenet_speech_amd.synthetic.ragged_reads on device="cpu") against
tests/golden/ragged_00.npz -- dwell, noise and signals the reference's own RawGaussianModelLoader / RawSignalGenerator produced
under a seeded numpy RNG (tests/golden/make_ragged_golden.py) -- the mirror of the loader class, and the chi-square yardstick
that tests/test_gpu_reads.py applies to the device's random dwell."""
import os

import numpy as np
import pytest
import torch

import wavenet_speech_amd as W
from wavenet_speech_amd import synthetic as S
from tests import dwell_stats as D
from tests.cpu_util import gold, ragged_table as _table  # noqa: F401


@pytest.mark.parametrize("case", ["case0", "case1", "case2"])
def test_torch_form_reproduces_the_reference_read(gold, case):
    g = lambda k: gold[case + "." + k]
    window = int(g("window"))
    bases, dwell, noise = torch.from_numpy(g("bases"))[None], torch.from_numpy(g("dwell"))[None], torch.from_numpy(g("noise"))[None]
    r = S.ragged_reads(1, window=window, table=_table(gold), bases=bases, dwell_values=dwell, noise=noise, device="cpu")
    n, K, L = bases.shape[1], dwell.shape[1], noise.shape[1]
    assert K == n - 4 - 2 * window
    assert r.signal.shape == (1, 1, L) and r.signal.dtype == torch.float32 and int(r.signal_lengths[0]) == L
    assert int(r.base_lengths[0]) == n and torch.equal(r.bases[0].long(), bases[0]) and torch.equal(r.targets.long(), bases[0])
    assert torch.equal(r.dwell[0].long(), dwell[0])
    assert torch.equal(r.starts[0].long(), torch.cat([torch.zeros(1, dtype=torch.long), dwell[0].cumsum(0)]))
    kmers = S.ragged_kmers(r.bases, r.base_lengths, window)
    assert torch.equal(kmers[0], torch.from_numpy(g("kmers")))
    assert torch.equal(kmers[0][r.sample_kmer[0].long()], torch.from_numpy(g("kmer_seq")))       # the k-mer of every sample, exactly
    assert torch.equal(r.signal[0, 0], torch.from_numpy(g("signal_f32")))                        # bit for bit


def test_torch_form_reproduces_the_reference_batch(gold):
    g = lambda k: torch.from_numpy(gold["batch." + k])
    r = S.ragged_reads(3, window="loader", table=_table(gold), bases=g("bases"), base_lengths=g("lengths"), dwell_values=g("dwell"),
                       noise=g("noise"), device="cpu")
    want = g("signal_f32")
    assert r.signal.shape == (3, 1, want.shape[1]) and torch.equal(r.signal[:, 0], want)
    assert torch.equal(r.signal_lengths.long(), g("signal_lengths")) and int(r.signal_lengths.max()) == want.shape[1]
    for b in range(3):
        n = int(r.signal_lengths[b])
        assert not r.signal[b, 0, n:].any() and bool((r.sample_kmer[b, n:] == -1).all()) and bool((r.sample_kmer[b, :n] >= 0).all())
        assert not r.bases[b, int(r.base_lengths[b]):].any()
    assert r.targets.dtype == torch.int32 and torch.equal(r.targets, g("seq"))
    assert r.base_lengths.dtype == torch.int32 and torch.equal(r.base_lengths, g("lengths"))
    assert int(r.targets.numel()) == int(r.base_lengths.sum())


def test_drawn_reads_are_consistent():
    gen = torch.Generator().manual_seed(5)
    for dwell, window in ((("uniform", 6, 2), "loader"), (("fixed", 3), "loader"), (("gamma", 2.461964, 587.2858, 4000.0), "generator"),
                          (("gamma", 0.5, 587.2858, 4000.0), "generator"), (("uniform", 1, 2), "loader")):
        r = W.ragged_reads(5, (20, 30), dwell, window, generator=gen)
        w = S.WINDOWS[window]
        K = r.base_lengths.long() - 4 - 2 * w
        assert int(r.base_lengths.min()) >= 20 and int(r.base_lengths.max()) < 30
        for b in range(5):
            k, n = int(K[b]), int(r.base_lengths[b])
            assert bool((r.dwell[b, :k] >= 1).all()) and not r.dwell[b, k:].any()
            assert bool(((r.bases[b, :n] >= 1) & (r.bases[b, :n] <= 4)).all()) and not r.bases[b, n:].any()
            assert int(r.signal_lengths[b]) == int(r.dwell[b].sum()) == int(r.starts[b, k])
            assert bool((r.starts[b, k:] == r.signal_lengths[b]).all())
            assert torch.equal(torch.bincount(r.sample_kmer[b, :int(r.signal_lengths[b])].long(), minlength=k), r.dwell[b, :k].long())
        if dwell[0] == "uniform":
            live = r.dwell[r.dwell > 0]
            assert int(live.min()) >= max(dwell[1] - dwell[2], 1) and int(live.max()) < dwell[1] + dwell[2]
    r = W.ragged_reads(2, (20, 30), ("fixed", 3), pad_to=100, generator=gen)
    assert r.signal.shape == (2, 1, 100)
    with pytest.raises(RuntimeError, match="pad_to"):
        W.ragged_reads(2, (20, 30), ("fixed", 3), pad_to=30, generator=gen)
    with pytest.raises(ValueError):
        W.ragged_reads(2, (20, 30), ("uniform", 1, 0))                 # [1, 1) is empty
    with pytest.raises(ValueError):
        W.ragged_reads(2, (8, 30), ("fixed", 3), "loader")             # a loader read needs 9 bases
    with pytest.raises(ValueError):
        W.ragged_reads(2, (20, 30), ("gamma", 0.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        W.ragged_reads(1, bases=torch.tensor([[1, 2, 3, 4, 5, 1, 2, 3, 4, 1]]))
    with pytest.raises(ValueError):
        W.ragged_reads(1, bases=torch.ones(1, 12, dtype=torch.long), dwell_values=torch.tensor([[2, 0, 2, 2]]))


def test_default_max_dwell():
    assert S.default_max_dwell(("fixed", 3)) == 3 and S.default_max_dwell(("uniform", 6, 2)) == 7
    m = S.default_max_dwell(("gamma", 2.461964, 587.2858, 4000.0))
    tail = lambda k: float(torch.special.gammaincc(torch.tensor(2.461964, dtype=torch.float64),
                                                   torch.tensor(587.2858 * k / 4000.0, dtype=torch.float64)))
    assert tail(m) < 1e-12 <= tail(m - 1)


def test_loader_mirror_counts_and_stops():
    ld = W.RawGaussianModelLoader(5, 2, 2, None, batch_size=3, upsampling=6, random_upsample=True, lengths=(20, 30))
    ld.generator = torch.Generator().manual_seed(3)
    assert (ld.counter, ld.epochs, ld.on_cuda) == (0, 0, False)
    sig, seq, lengths = ld.fetch()
    assert sig.dim() == 2 and sig.shape[0] == 3 and sig.dtype == torch.float32
    assert seq.dtype == torch.int32 and lengths.dtype == torch.int32 and seq.numel() == int(lengths.sum())
    assert int(lengths.min()) >= 20 and int(lengths.max()) < 30 and (ld.counter, ld.epochs) == (1, 0)
    ld.fetch()
    assert (ld.counter, ld.epochs) == (2, 1)
    reads = ld.fetch_reads()
    assert isinstance(reads, W.RaggedReads) and (ld.counter, ld.epochs) == (3, 1)
    live = reads.dwell[reads.dwell > 0]
    assert int(live.min()) >= 4 and int(live.max()) <= 7
    ld.fetch()
    assert (ld.counter, ld.epochs) == (4, 2)
    with pytest.raises(StopIteration):                                 # epochs == num_epochs before max_iters
        ld.fetch()
    ld = W.RawGaussianModelLoader(2, 10, 10, None, upsampling=3)
    assert ld.fetch_reads().dwell.max() == 3                           # random_upsample=False: every k-mer held 3 samples
    ld.fetch()
    with pytest.raises(StopIteration):                                 # counter == max_iters
        ld.fetch()
    assert (ld.counter, ld.epochs) == (2, 0)
    ld.cuda()
    assert ld.on_cuda
    ld.cpu()
    assert not ld.on_cuda


def test_loader_reads_a_table_file(tmp_path, gold):
    path = os.path.join(str(tmp_path), "table.npz")
    np.savez(path, means=gold["table.means"], stdvs=gold["table.stdvs"])
    ld = W.RawGaussianModelLoader(10, 1, 10, path, batch_size=2, upsampling=6, random_upsample=True)
    assert torch.equal(ld.kmer_means, torch.from_numpy(gold["table.means"]))
    reads = ld.fetch_reads()
    kmers = S.ragged_kmers(reads.bases, reads.base_lengths, 2)
    n = int(reads.signal_lengths[0])
    k = kmers[0][reads.sample_kmer[0, :n].long()]
    z = (reads.signal[0, 0, :n].double() - ld.kmer_means[k]) / ld.kmer_stdvs[k]
    assert float(z.abs().max()) < 6.0                                  # every sample near its own k-mer's mean


N_DRAWS = 200000


def test_yardstick_accepts_the_reference_formulas_and_rejects_near_misses():
    np.random.seed(11)
    uni = np.random.randint(low=max(6 - 2, 1), high=6 + 2, size=N_DRAWS)
    assert D.accepts(torch.from_numpy(uni), D.uniform_pmf(6, 2))
    assert not D.accepts(torch.from_numpy(uni), D.uniform_pmf(6, 3))           # w + 1: another interval
    wide = np.random.randint(low=max(6 - 3, 1), high=6 + 3, size=N_DRAWS)
    assert not D.accepts(torch.from_numpy(wide), D.uniform_pmf(6, 2))          # draws outside the support
    for shape in (2.461964, 0.5):
        n = (np.random.gamma(shape, np.reciprocal(587.2858), size=N_DRAWS) * 4000.0).astype(np.int32)
        n = n + (n == 0).astype(np.int32)
        pmf = D.gamma_floor_pmf(shape, 587.2858, 4000.0)
        assert abs(float(pmf[1].sum()) - 1.0) < 1e-12
        stat, dof, outside = D.chi_square(torch.from_numpy(n), pmf)
        print("gamma shape %g: chi2 %.1f, dof %d, bound %.1f" % (shape, stat, dof, D.chi_square_quantile(dof)))
        assert D.accepts(torch.from_numpy(n), pmf)
        assert not D.accepts(torch.from_numpy(n), D.gamma_floor_pmf(shape * 1.05, 587.2858, 4000.0))
    # Wilson-Hilferty against the exact 1 - 1e-6 quantiles of chi-square: 30.665 (3 dof, where it is 7 % loose), 112.608 (50),
    # 247.153 (150)
    assert 30.665 < D.chi_square_quantile(3) < 30.665 * 1.08
    assert 112.608 < D.chi_square_quantile(50) < 112.608 * 1.005 and 247.153 < D.chi_square_quantile(150) < 247.153 * 1.002
