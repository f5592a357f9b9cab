"""The inputs of the read-statistics tests, shared by tests/test_read_stats_ref.py (CPU, the numpy restatement against np.sort) and
tests/test_gpu_normalise.py (GPU, the kernels against np.sort and the restatement): numpy arrays only, built once per process."""
import functools

import numpy as np

from wavenet_speech_amd.normalise import TILE as T

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 5)
PATTERN_N = 1003               # one read per value pattern: odd, no multiple of a vector or a wave


def _batch(reads, dtype, ld, garbage):
    """[B, ld] with read b in row b and the two garbage values alternating past its length"""
    x = np.empty((len(reads), ld), dtype=dtype)
    x[:, 0::2] = garbage[0]
    x[:, 1::2] = garbage[1]
    for b, r in enumerate(reads):
        x[b, :len(r)] = r
    return x, np.array([len(r) for r in reads], dtype=np.int32)


def _garbage(dtype):
    return (32767, -32768) if dtype == np.int16 else (np.float32(np.inf), np.float32(-np.inf))


@functools.lru_cache(maxsize=None)
def ragged(dtype_name):
    """(x [13, ld], lengths): reads of SIZES samples; ld = 2 T + 7 is odd, so int16 rows start 2-byte aligned only"""
    dtype = np.dtype(dtype_name).type
    rng = np.random.default_rng(5)
    reads = []
    for i, n in enumerate(SIZES):
        if dtype == np.int16:
            r = rng.integers(-32768, 32768, n) if i % 2 else np.clip(np.rint(rng.normal(500.0, 30.0, n)), -32768, 32767)
        else:
            r = rng.normal(0.0, 1.0, n) * (10.0 ** rng.integers(-3, 4, n)) if i % 2 else np.rint(rng.normal(90.0, 12.0, n) * 4) / 4
        reads.append(r.astype(dtype))
    return _batch(reads, dtype, 2 * T + 7, _garbage(dtype))


@functools.lru_cache(maxsize=None)
def int16_patterns():
    """(names, x [7, ld], lengths): value patterns that exercise each of the two digits"""
    rng = np.random.default_rng(6)
    n = PATTERN_N
    reads = {
        "all_equal": np.full(n, -1234),
        "two_values": rng.choice([17, 300], n),
        "extremes": rng.choice([-32768, 32767], n),
        "low_byte_only": 0x1200 + rng.integers(0, 256, n),
        "high_byte_only": (rng.integers(-128, 128, n) << 8) | 0x5A,
        "concentrated": np.clip(np.rint(rng.normal(500.0, 30.0, n)), -32768, 32767),
        "uniform": rng.integers(-32768, 32768, n),
    }
    x, lengths = _batch([r.astype(np.int16) for r in reads.values()], np.int16, n + 2, _garbage(np.int16))
    return tuple(reads), x, lengths


@functools.lru_cache(maxsize=None)
def fp32_patterns():
    """(names, x [8, ld], lengths): the last read holds one positive NaN"""
    rng = np.random.default_rng(7)
    n = PATTERN_N
    bits = lambda u: np.asarray(u, dtype=np.uint32).view(np.float32)                     # noqa: E731
    zeros = np.where(rng.integers(0, 2, n) == 1, np.float32(0.0), np.float32(-0.0))
    infs = rng.choice(np.array([np.inf, -np.inf, 1.5, -2.5], dtype=np.float32), n)
    reads = {
        "mixed_signs": rng.normal(0.0, 100.0, n),
        "signed_zeros": np.concatenate([zeros[:n - 2], [-1e-30, 1e-30]]),
        "infinities": infs,
        "denormals": bits(rng.integers(0, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)),
        "duplicates": rng.choice(np.array([-3.25, 0.5, 0.5, 7.0, 7.0, 7.0], dtype=np.float32), n),
        "low_mantissa_byte": bits(np.uint32(0x42F6E900) + rng.integers(0, 256, n).astype(np.uint32)),
        "exponent_only": bits((rng.integers(1, 255, n).astype(np.uint32) << 23) | np.uint32(0x00400000)),
        "one_nan": np.concatenate([rng.normal(0.0, 1.0, n - 1), [np.nan]]),
    }
    x, lengths = _batch([np.asarray(r, dtype=np.float32) for r in reads.values()], np.float32, n + 2, _garbage(np.float32))
    assert not np.signbit(x[-1, n - 1]) and np.isnan(x[-1, n - 1])
    return tuple(reads), x, lengths


def edge_ranks(lengths, K, seed):
    """[B, K] int32: 0, n - 1, (n - 1) // 2, n // 2, then random ranks; K = 1: one random rank"""
    rng = np.random.default_rng(seed)
    out = np.empty((len(lengths), K), dtype=np.int32)
    for b, n in enumerate(int(v) for v in lengths):
        fixed = [0, n - 1, (n - 1) // 2, n // 2] if K > 1 else []
        out[b] = (fixed + [int(v) for v in rng.integers(0, n, K)])[:K]
    return out


def sweep_ranks(lengths, K, call, seed):
    """[B, K] int32 for call number `call`: reads of up to K (call + 1) samples walk through their ranks K at a time (wrapping), so
    ceil(n / K) calls give a read of n samples every rank; longer reads get random ranks"""
    rng = np.random.default_rng(seed + call)
    out = np.empty((len(lengths), K), dtype=np.int32)
    for b, n in enumerate(int(v) for v in lengths):
        out[b] = (np.arange(K * call, K * (call + 1)) % n) if n <= 65 else rng.integers(0, n, K)
    return out


def deviation_centers(dtype, B):
    """[B] float32: integer, half-integer and arbitrary centres in turn"""
    base = np.array([500.0, 499.5, 498.7654], dtype=np.float32) if dtype == np.int16 else np.array([90.0, 0.5, 0.1234567], dtype=np.float32)
    return np.resize(base, B).astype(np.float32)


def sorted_reads(x, lengths, centers=None):
    """np.sort of every read (of its float32 deviations from centers[b]); NaN last, as in torch.sort"""
    out = []
    for b, n in enumerate(int(v) for v in lengths):
        r = x[b, :n]
        if centers is not None:
            r = np.abs(r.astype(np.float32) - np.float32(centers[b])).astype(np.float32)
        out.append(np.sort(r))
    return out


def pick(sorted_rows, ranks):
    """[B, K] float32: sorted_rows[b][ranks[b][k]]"""
    return np.array([[np.float32(row[r]) for r in rk] for row, rk in zip(sorted_rows, ranks)], dtype=np.float32)
