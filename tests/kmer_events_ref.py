"""The definition of wn_kmer_events (include/wavenet_amd.h) as a plain loop with Python integers: event table, per-read counts,
k-mer tables.  Floating point enters once per sample, v = x * scale + shift in float64 (the product is exact, so there is one
rounding), then q = round-half-even(v * 2^F); everything after that is integer.  numpy is used to hold arrays, not to sum."""
import math

import numpy as np

MAX_EVENT = 65536
Q_LIMIT = 1 << 23


def quantise(x, scale_shift, frac_bits):
    """q of one sample, or None when it is not finite or |q| >= 2^23"""
    v = float(x)
    if scale_shift is not None:
        v = v * float(scale_shift[0]) + float(scale_shift[1])        # 24 x 24 bits: the product is exact in float64
    s = v * float(1 << frac_bits)                                    # exact, or inf
    if not math.isfinite(s):
        return None
    q = round(s)                                                     # Python rounds a float half to even, to an exact integer
    return q if abs(q) < Q_LIMIT else None


def kmer_index(window):
    idx = 0
    for v in window:
        idx = idx * 4 + (int(v) - 1)
    return idx


def read_events(signal, n, labels, ll, begin, end, ne, k, first, frame_stride, frame_offset, scale_shift, frac_bits, max_signal,
                max_labels):
    """one read -> None when it is bad, else the list of (code, start, length, sum, sumsq) of its first ne events"""
    N = len(begin)
    if not (0 <= n <= max_signal and 0 <= ll <= max_labels and 0 <= ne <= N):
        return None
    out = []
    for j in range(ne):
        bg, en = int(begin[j]), int(end[j])
        if bg < 0 or en < bg or (j > 0 and bg < int(end[j - 1])):
            return None
        s0, s1 = bg * frame_stride + frame_offset, en * frame_stride + frame_offset
        c0, c1 = min(s0, n), min(s1, n)
        length = c1 - c0
        w0 = j + first
        if length == 0:
            out.append((-2, c0, 0, 0, 0))
        elif s1 > n or length > MAX_EVENT:
            out.append((-3, c0, length, 0, 0))
        elif w0 < 0 or w0 + k > ll:
            out.append((-1, c0, length, 0, 0))
        else:
            window = [int(v) for v in labels[w0:w0 + k]]
            if any(v < 1 or v > 4 for v in window):
                return None
            total, squares = 0, 0
            for x in signal[c0:c1].tolist():
                q = quantise(x, scale_shift, frac_bits)
                if q is None:
                    return None
                total += q
                squares += q * q
            out.append((kmer_index(window), c0, length, total, squares))
    return out


def kmer_events_ref(signal, signal_lengths, labels, label_lengths, begin, end, events, k=5, first=-2, frame_stride=1, frame_offset=0,
                    scale_shift=None, frac_bits=12, max_dwell=255, tables=None):
    """signal [B, L] float32 or int16; labels [B, n]; begin, end [B, N]; events [B].  tables: (kmer_stats, dwell_hist) to add into
    (lists of lists of Python integers, changed in place) or None for fresh ones.  Returns a dict of numpy arrays (int64 for the
    sums; the tables as object arrays of Python integers) and `bad`, the number of bad reads."""
    B, N = np.asarray(begin).shape
    L, n_lab = signal.shape[1], np.asarray(labels).shape[1]
    kmer = np.full((B, N), -4, dtype=np.int32)
    start, length = np.zeros((B, N), dtype=np.int32), np.zeros((B, N), dtype=np.int32)
    total, squares = np.zeros((B, N), dtype=np.int64), np.zeros((B, N), dtype=np.int64)
    read_counts = np.full((B, 4), -1, dtype=np.int32)
    stats, hist = tables if tables is not None else ([[0] * 5 for _ in range(4 ** k)], [[0] * (max_dwell + 1) for _ in range(4 ** k)])
    bad = 0
    for b in range(B):
        ss = None if scale_shift is None else scale_shift[b]
        rows = read_events(signal[b], int(signal_lengths[b]), labels[b], int(label_lengths[b]), begin[b], end[b], int(events[b]), k,
                           first, frame_stride, frame_offset, ss, frac_bits, L, n_lab)
        if rows is None:
            bad += 1
            continue
        counts = [0, 0, 0, 0]
        for j, (code, c0, n, s1, s2) in enumerate(rows):
            kmer[b, j], start[b, j], length[b, j], total[b, j], squares[b, j] = code, c0, n, s1, s2
            if code >= 0:
                counts[0] += 1
                counts[3] += n
                row = stats[code]
                row[0] += 1
                row[1] += n
                row[2] += s1
                row[3] += s2 & 0xffffffff
                row[4] += s2 >> 32
                hist[code][min(n, max_dwell)] += 1
            else:
                counts[1 if code == -1 else 2] += 1
        read_counts[b] = counts
    return {"kmer": kmer, "start": start, "length": length, "sum": total, "sumsq": squares, "read_counts": read_counts,
            "kmer_stats": np.array(stats, dtype=np.int64), "dwell_hist": np.array(hist, dtype=np.int64), "bad": bad,
            "tables": (stats, hist)}
