"""Reference for the per-base qualities of a decoded read: a float64 restatement of the definitions in
plain Python loops over numpy scalars -- no torch, no vectorised shortcuts that could share a mistake with the kernel.

For utterance b with T_b frames and class values x_t(c):
    w_t(c)   = exp(x_t(c) - max_c x_t(c)) for "logits" and "log_probs", x_t(c) for "probs"
    eps_t(l) = sum_{c != l} w_t(c) / sum_c w_t(c)                         (never 1 - p)
    a_t      = the lowest class among the maxima of x_t (strict >)
    run of base j (label l, frame f): f, then t = f + 1, ... < min(frame of base j + 1, T_b) (T_b for the last base) while a_t == l
    e_j      = mean of eps_t(l) over the run ("mean") or its minimum ("best"); dwell_j = frames in the run
    Q_j      = qscale * (-10 log10 e_j) + qbias, qual_j = clamp(floor(Q_j + 0.5), 0, 93), NaN -> 0
    read_error = mean of e_j over the read's bases, NaN for an empty read
A base is bad (e NaN, qual 0, dwell 0, read_error NaN, counted) when its label is outside [0, C) or the blank, its frame is
outside [0, T_b) or not above its predecessor's; a read whose length is outside [0, Lmax] or whose input length is outside
[0, T] is bad as a whole and counts once."""
import math

import numpy as np

KINDS = ("logits", "probs", "log_probs")
STATS = ("mean", "best")
MAX_QUAL = 93


def frame_argmax(col):
    """lowest class among the maxima of one frame (strict >, as the greedy decoder)"""
    best, m = 0, col[0]
    for c in range(1, len(col)):
        if col[c] > m:
            best, m = c, col[c]
    return best


def frame_error(col, label, kind="logits"):
    """eps_t(label) of one frame col [C] in float64"""
    col = [float(v) for v in col]
    if kind == "probs":
        w = col
    else:
        m = col[frame_argmax(col)]
        w = [math.exp(v - m) for v in col]
    total, others = 0.0, 0.0
    for c, v in enumerate(w):
        total += v
        if c != label:
            others += v
    return others / total if total != 0.0 else float("nan")


def phred(e, qscale=1.0, qbias=0.0):
    """(Q, qual) of an error probability"""
    if math.isnan(e) or e < 0.0:
        return float("nan"), 0
    if e == 0.0:
        return float("inf"), MAX_QUAL
    q = qscale * (-10.0 * math.log10(e)) + qbias
    if math.isinf(q):
        return q, MAX_QUAL if q > 0 else 0
    return q, int(min(max(math.floor(q + 0.5), 0), MAX_QUAL))


def read_qualities(x, labels, frames, input_length=None, blank=0, kind="logits", stat="mean", qscale=1.0, qbias=0.0):
    """one read: x [C, T], labels / frames: sequences of its bases.  Returns (error, Q, qual, dwell: lists over the bases,
    read_error, number of bad bases)."""
    assert kind in KINDS and stat in STATS
    x = np.asarray(x, dtype=np.float64)
    C, T = x.shape
    tb = T if input_length is None else int(input_length)
    n = len(labels)
    error, Q, qual, dwell, bad = [], [], [], [], 0
    for j in range(n):
        l, f = int(labels[j]), int(frames[j])
        wrong = l < 0 or l >= C or l == blank or f < 0 or f >= tb or (j > 0 and f <= int(frames[j - 1]))
        if wrong:
            bad += 1
            error.append(float("nan")); Q.append(float("nan")); qual.append(0); dwell.append(0)
            continue
        lim = tb if j + 1 == n else min(int(frames[j + 1]), tb)
        eps = [frame_error(x[:, f], l, kind)]
        t = f + 1
        while t < lim and frame_argmax(x[:, t]) == l:
            eps.append(frame_error(x[:, t], l, kind))
            t += 1
        if stat == "mean":
            s = 0.0
            for v in eps:                                            # in frame order
                s += v
            e = s / len(eps)
        else:
            e = min(eps)
        q, k = phred(e, qscale, qbias)
        error.append(e); Q.append(q); qual.append(k); dwell.append(len(eps))
    if n == 0:
        read_error = float("nan")
    else:
        s = 0.0
        for v in error:
            s += v
        read_error = s / n
    return error, Q, qual, dwell, read_error, bad


def batch_qualities(x, labels, frames, lengths, input_lengths=None, blank=0, kind="logits", stat="mean", qscale=1.0, qbias=0.0):
    """x [B, C, T], labels / frames [B, Lmax], lengths [B] -> dict of error, Q [B, Lmax] float64 (NaN at and past the length),
    qual, dwell [B, Lmax] int64 (0 there), read_error [B] float64, bad: the count the device flag holds"""
    x = np.asarray(x)
    labels, frames, lengths = np.asarray(labels), np.asarray(frames), np.asarray(lengths)
    B, C, T = x.shape
    lmax = labels.shape[1]
    out = dict(error=np.full((B, lmax), np.nan), Q=np.full((B, lmax), np.nan), qual=np.zeros((B, lmax), dtype=np.int64),
               dwell=np.zeros((B, lmax), dtype=np.int64), read_error=np.full(B, np.nan), bad=0)
    for b in range(B):
        n = int(lengths[b])
        tb = T if input_lengths is None else int(input_lengths[b])
        if n < 0 or n > lmax or tb < 0 or tb > T:
            out["bad"] += 1                                          # the whole read, once
            continue
        e, q, k, d, re, bad = read_qualities(x[b], labels[b, :n], frames[b, :n], tb, blank, kind, stat, qscale, qbias)
        out["error"][b, :n], out["Q"][b, :n], out["qual"][b, :n], out["dwell"][b, :n] = e, q, k, d
        out["read_error"][b] = re
        out["bad"] += bad
    return out
