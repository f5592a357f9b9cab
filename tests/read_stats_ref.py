"""numpy restatement of the read statistics of wavenet_speech_amd/normalise.py and csrc/wn_select.hip: the order-preserving keys,
the most-significant-digit selection pass by pass (histogram of one digit among the elements that share the prefix, the chosen
digit, the remaining rank), the deviation mode, the med / MAD midpoint rule and the quantile rank arithmetic.  Written from the
definitions, one read at a time, with no sort anywhere: tests/test_read_stats_ref.py holds it to np.sort and np.median, the GPU
tests hold the kernels to it and to np.sort."""
import numpy as np

DIGIT_BITS = 8


def keys(x, center=None):
    """(unsigned keys, bits per key) of a 1-D int16 or float32 array; with center (a float32 scalar) of the deviations
    |float32(x) - center| rounded once to float32"""
    x = np.asarray(x)
    if center is not None:
        d = np.abs(x.astype(np.float32) - np.float32(center)).astype(np.float32)
        return d.view(np.uint32), 32
    if x.dtype == np.int16:
        return (x.view(np.uint16) ^ np.uint16(0x8000)).astype(np.uint32), 16
    assert x.dtype == np.float32, x.dtype
    u = x.view(np.uint32)
    return u ^ np.where(u >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)), 32


def value_of_key(key, dtype, deviation):
    """the element a key stands for, as float32: the inverse of keys()"""
    key = np.uint32(key)
    if deviation:
        return np.array([key], dtype=np.uint32).view(np.float32)[0]
    if np.dtype(dtype) == np.int16:
        return np.float32(np.array([key ^ np.uint32(0x8000)], dtype=np.uint32).astype(np.uint16).view(np.int16)[0])
    u = key ^ (np.uint32(0x80000000) if key >> np.uint32(31) else np.uint32(0xFFFFFFFF))
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def select_key(k, bits, rank):
    """the rank-th smallest (0-based) of the keys k by digits, most significant first; also the histogram trace
    [(prefix, histogram, digit, remaining rank)] of every pass"""
    assert 0 <= rank < len(k)
    prefix, rem, trace = 0, int(rank), []
    for p in range(bits // DIGIT_BITS):
        shift = bits - DIGIT_BITS * (p + 1)
        live = k if p == 0 else k[(k >> np.uint32(shift + DIGIT_BITS)) == np.uint32(prefix)]
        hist = np.bincount(((live >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        below = np.cumsum(hist) - hist                        # counts of the bins below each digit
        digit = int(np.nonzero(below <= rem)[0][-1])          # the last bin that starts at or before the remaining rank
        assert hist[digit] > 0 and rem < below[digit] + hist[digit]
        rem -= int(below[digit])
        trace.append((prefix, hist, digit, rem))
        prefix = (prefix << DIGIT_BITS) | digit
    return np.uint32(prefix), trace


def order_statistic(x, n, rank, center=None):
    """float32: the rank-th smallest of x[:n] (of its deviations from center); 0.0 for a refused (n, rank), as the kernels"""
    x = np.asarray(x)
    if n < 0 or n > len(x) or rank < 0 or rank >= n:
        return np.float32(0.0)
    k, bits = keys(x[:n], center)
    key, _ = select_key(k, bits, rank)
    return value_of_key(key, x.dtype, center is not None)


def midpoint(a, b):
    return np.float32(np.float32(np.float32(a) + np.float32(b)) * np.float32(0.5))


def med_mad(x, n):
    """(med, mad) float32 of x[:n], n >= 1: midpoints of the order statistics at ranks (n - 1) // 2 and n // 2, of the samples and
    of their deviations from med"""
    r = ((n - 1) // 2, n // 2)
    med = midpoint(order_statistic(x, n, r[0]), order_statistic(x, n, r[1]))
    mad = midpoint(order_statistic(x, n, r[0], med), order_statistic(x, n, r[1], med))
    return med, mad


def quantile_ranks(n, q):
    """(pos, lo, hi): pos = q (n - 1) in float64, lo = floor(pos), hi = ceil(pos) (= min(lo + 1, n - 1) wherever pos has a fraction)"""
    pos = np.float64(q) * np.float64(n - 1)
    return pos, int(np.floor(pos)), int(np.ceil(pos))


def quantile(x, n, q, interpolation="linear"):
    pos, lo, hi = quantile_ranks(n, q)
    v_lo, v_hi = order_statistic(x, n, lo), order_statistic(x, n, hi)
    if interpolation == "lower":
        return v_lo
    if interpolation == "higher":
        return v_hi
    if interpolation == "midpoint":
        return midpoint(v_lo, v_hi)
    assert interpolation == "linear", interpolation
    return np.float32(np.float64(v_lo) + (np.float64(v_hi) - np.float64(v_lo)) * (pos - lo))


def medmad_normalisation(x, n):
    """(scale, shift) float32: shift = -med, scale = 1 / (1.4826f mad), 1 where mad == 0"""
    med, mad = med_mad(x, n)
    scale = np.float32(1.0) if mad == 0 else np.float32(1.0) / np.float32(mad * np.float32(1.4826))
    return np.float32(scale), np.float32(-med)
