#!/usr/bin/env python3
"""
Writes tests/golden/ragged_00.npz: golden vectors of the reference's RAGGED generators, captured by importing
/root/reference/utils/gaussian_kmer_model.py (RawGaussianModelLoader, random_upsample at :316-319, called from :231) and
/root/reference/utils/raw_signal_generator.py (RawSignalGenerator.gaussian_model_fn, random_upsample at :189-203, called from
:111) in the build container and calling their own code under a seeded numpy global RNG.  The reference draws the dwell and
the noise itself; this script REPLAYS the same draws from the same seed (np.random.randint / np.random.gamma, then
np.random.standard_normal) and asserts that the replay reproduces what the reference computed, so the fixture can hold the
dwell and the noise as inputs of a deterministic check:

    case0  loader, random_upsample=True, upsampling 6 (uniform dwell in [4, 8)), window [4:-4]
    case1  loader, random_upsample=False, upsampling 3 (fixed dwell), window [4:-4]
    case2  RawSignalGenerator, gamma dwell with the default shape / rate at sample_rate 4000, window [2:-2]
    batch  one seeded RawGaussianModelLoader.fetch() of 3 reads: padded signal, concatenated seq, lengths

raw_signal_generator.py imports h5py at module level (for the reference genome, not mirrored); an empty placeholder module of
that name is put into sys.modules first.  Only module-level functions and gaussian_model_fn on an object.__new__ instance are
used.  The 1024-entry mean/stdv table is synthetic (seeded), not the reference's nanopolish table.  The reference itself never
travels: only these numbers are committed.

    python tests/golden/make_ragged_golden.py
"""
import os
import sys
import tempfile
import types
import warnings

import numpy as np

REF = "/root/reference"
sys.path.insert(0, REF)
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
sys.modules.setdefault("h5py", types.ModuleType("h5py"))
from scipy.ndimage import generic_filter  # noqa: E402
try:
    import scipy.ndimage.filters  # noqa: E402,F401
except ImportError:                                   # the deprecated namespace raw_signal_generator.py imports from
    _m = types.ModuleType("scipy.ndimage.filters")
    _m.generic_filter = generic_filter
    sys.modules["scipy.ndimage.filters"] = _m
from utils import gaussian_kmer_model as GK  # noqa: E402
from utils import raw_signal_generator as RG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = np.array([256, 64, 16, 4, 1])


def replay_noise(mean, stdv, signal):
    """np.random.normal(loc, scale) draws one standard normal per element: replay it; if loc + scale * z does not reproduce the
    reference bit for bit, recover z from the signal instead (and hold it to 1e-12)"""
    z = np.random.standard_normal(size=signal.shape)
    if np.array_equal(mean + stdv * z, signal):
        return z, True
    z2 = (signal - mean) / stdv
    assert np.abs(z2 - z).max() < 1e-12, np.abs(z2 - z).max()
    assert np.array_equal(mean + stdv * z2, signal), "neither the replayed nor the recovered noise reproduces the signal"
    return z2, False


def one_read(out, pre, model, bases, window, seed, draw_dwell, means, stdvs):
    """run model.gaussian_model_fn(bases) under `seed`, then replay its draws"""
    np.random.seed(seed)
    signal = model.gaussian_model_fn(bases)
    kmers = generic_filter(bases, model.nts_to_kmer, size=(5,), mode='constant')
    kmers = (kmers[4:-4] if window == 2 else kmers[2:-2]).astype(np.int64)
    # the windows, restated: k-mer p = bases[p + window .. p + window + 4]
    assert np.array_equal(kmers, np.array([((bases[p + window:p + window + 5] - 1) * WEIGHTS).sum() for p in range(len(kmers))]))
    np.random.seed(seed)
    dwell = draw_dwell(kmers.shape)
    kmer_seq = np.repeat(kmers, dwell)
    assert kmer_seq.shape == signal.shape, (kmer_seq.shape, signal.shape)      # the replayed dwell is the reference's
    noise, bitwise = replay_noise(means[kmer_seq], stdvs[kmer_seq], signal)
    out.update({pre + "bases": bases.astype(np.int64), pre + "window": np.int64(window), pre + "dwell": dwell.astype(np.int64),
                pre + "kmers": kmers, pre + "kmer_seq": kmer_seq, pre + "noise": noise, pre + "signal": signal,
                pre + "signal_f32": signal.astype(np.float32)})
    return bitwise


def main():
    rng = np.random.RandomState(20260102)
    means = 59.6 + (118.5 - 59.6) * rng.rand(1024)
    stdvs = 1.34 + (5.86 - 1.34) * rng.rand(1024)
    out = {"table.means": means, "table.stdvs": stdvs}
    bitwise = []
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "table.npz")
        np.savez(table, means=means, stdvs=stdvs)

        # case0: the loader's uniform dwell
        ld = GK.RawGaussianModelLoader(10, 1, 10, table, batch_size=1, upsampling=6, random_upsample=True, lengths=(20, 30))
        bases = rng.randint(1, 5, size=173)
        bitwise.append(one_read(out, "case0.", ld, bases, 2, 101, lambda shape: np.random.randint(low=max(6 - 2, 1), high=6 + 2, size=shape),
                                means, stdvs))
        out["case0.dwell_model"] = np.array([6, 2], dtype=np.int64)

        # case1: the loader's fixed dwell
        ld = GK.RawGaussianModelLoader(10, 1, 10, table, batch_size=1, upsampling=3, random_upsample=False, lengths=(20, 30))
        bases = rng.randint(1, 5, size=96)
        bitwise.append(one_read(out, "case1.", ld, bases, 2, 102, lambda shape: np.full(shape, 3, dtype=np.int64), means, stdvs))
        out["case1.dwell_model"] = np.array([3], dtype=np.int64)

        # case2: RawSignalGenerator's gamma dwell (defaults 2.461964 / 587.2858) at sample_rate 4000
        gen = object.__new__(RG.RawSignalGenerator)
        gen.kmer_means, gen.kmer_stdvs = means, stdvs
        gen.duration_shape, gen.duration_rate, gen.sample_rate = 2.461964, 587.2858, 4000.

        def gamma_dwell(shape):
            n = (np.random.gamma(2.461964, np.reciprocal(587.2858), size=shape) * 4000.).astype(np.int32)
            return n + (n == 0).astype(np.int32)
        bases = rng.randint(1, 5, size=200)
        bitwise.append(one_read(out, "case2.", gen, bases, 0, 103, gamma_dwell, means, stdvs))
        out["case2.dwell_model"] = np.array([2.461964, 587.2858, 4000.])

        # batch: one fetch() of three reads, and the replay of everything it drew
        ld = GK.RawGaussianModelLoader(10, 1, 10, table, batch_size=3, upsampling=6, random_upsample=True, lengths=(20, 30))
        np.random.seed(104)
        signal, seq, lengths = ld.fetch()
        signal, seq, lengths = signal.numpy(), seq.numpy(), lengths.numpy()
        assert ld.counter == 1 and signal.dtype == np.float32 and seq.dtype == np.int32 and lengths.dtype == np.int32
        np.random.seed(104)
        lens = np.random.choice(range(20, 30), size=3)
        seqs = [np.random.randint(1, high=5, size=k, dtype=np.int32) for k in lens]
        assert np.array_equal(lens, lengths) and np.array_equal(np.concatenate(seqs), seq)
        nmax, kmax = int(lens.max()), int(lens.max()) - 8
        b_pad, d_pad = np.zeros((3, nmax), np.int64), np.zeros((3, kmax), np.int64)
        z_pad, s64 = np.zeros((3, signal.shape[1])), np.zeros((3, signal.shape[1]))
        sig_lengths = []
        for i, sq in enumerate(seqs):
            kmers = generic_filter(sq, ld.nts_to_kmer, size=(5,), mode='constant')[4:-4].astype(int)
            dwell = np.random.randint(low=4, high=8, size=kmers.shape)
            kmer_seq = np.repeat(kmers, dwell)
            z = np.random.standard_normal(size=kmer_seq.shape)
            x = means[kmer_seq] + stdvs[kmer_seq] * z
            n = x.shape[0]
            if not np.array_equal(x.astype(np.float32), signal[i, :n]):
                raise AssertionError("the replay of fetch() does not reproduce its signal")
            assert not signal[i, n:].any()                                  # batchify: zero padding
            b_pad[i, :len(sq)], d_pad[i, :len(dwell)], z_pad[i, :n], s64[i, :n] = sq, dwell, z, x
            sig_lengths.append(n)
        assert max(sig_lengths) == signal.shape[1]
        out.update({"batch.signal_f32": signal, "batch.seq": seq, "batch.lengths": lengths, "batch.bases": b_pad, "batch.dwell": d_pad,
                    "batch.noise": z_pad, "batch.signal": s64, "batch.signal_lengths": np.array(sig_lengths, dtype=np.int64)})
    np.savez_compressed(os.path.join(HERE, "ragged_00.npz"), **out)
    print("wrote ragged_00.npz; noise replayed bitwise:", bitwise)
    print({k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
