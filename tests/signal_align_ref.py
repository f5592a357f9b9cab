"""The definition of wn_signal_align (include/wavenet_amd.h) on the host: the banded minimum-cost stay / step path of the samples of
a read over the k-mers of its known bases.  Samples are quantised as wn_kmer_events does (tests/kmer_events_ref.quantise); every
number after that is an integer.  `sample_cost` is the definition in Python integers; `cost_row` is the same number for a row of
states in numpy uint64 (the product split at bit 24, so nothing exceeds 64 bits) and is held to `sample_cost` by
tests/test_signal_align_ref.py.  The dynamic program walks the samples in a Python loop with one numpy row per sample."""
import numpy as np

from tests.kmer_events_ref import kmer_index, quantise

INF = 1 << 62
NO_ALIGNMENT = (1 << 63) - 1            # LLONG_MAX
BAD_READ = -(1 << 63)                   # LLONG_MIN
Q_LIMIT = 1 << 23
OFFSET_LIMIT = 1 << 30


def sample_cost(q, level, weight, offset, S, max_cost):
    """min((d d weight) >> S, max_cost) + offset, d = |q - level|, in Python integers"""
    d = abs(int(q) - int(level))
    return min((d * d * int(weight)) >> S, int(max_cost)) + int(offset)


def cost_row(q, level, weight, offset, S, max_cost):
    """sample_cost of one q against arrays of model rows: int64 array.  d d = A 2^24 + B with A, B < 2^24; A w and B w stay below
    2^55; floor((A w 2^24 + B w) / 2^S) = floor(U / 2^(S - 24)) with U = A w + (B w >> 24) for S >= 24, and
    (U << (24 - S)) + ((B w mod 2^24) >> S) for 16 <= S < 24 (U < 2^55, so the shift stays below 2^63)"""
    d = np.abs(np.int64(q) - level.astype(np.int64)).astype(np.uint64)
    dd = d * d
    w = weight.astype(np.uint64)
    aw, bw = (dd >> np.uint64(24)) * w, (dd & np.uint64(0xffffff)) * w
    u = aw + (bw >> np.uint64(24))
    if S >= 24:
        sh = u >> np.uint64(S - 24)
    else:
        sh = (u << np.uint64(24 - S)) + ((bw & np.uint64(0xffffff)) >> np.uint64(S))
    return np.minimum(sh, np.uint64(max_cost)).astype(np.int64) + offset.astype(np.int64)


def band_centre(t, N, T):
    return ((2 * t + 1) * N) // (2 * T)


def band_lo(t, N, T, W):
    return min(max(band_centre(t, N, T) - W // 2, 0), max(N - W, 0))


def read_states(labels, ll, k, first):
    """the k-mer index of every state of a read, or None when a label of the used window is outside 1..4"""
    N = ll - (k - 1) - 2 * first
    used = [int(v) for v in labels[first:first + N + k - 1]]
    if any(v < 1 or v > 4 for v in used):
        return None
    return [kmer_index(used[j:j + k]) for j in range(N)]


def read_samples(signal, T, scale_shift, frac_bits):
    """q of the samples [0, T), or None when one of them is not finite or out of range"""
    out = []
    for x in signal[:T].tolist():
        q = quantise(x, scale_shift, frac_bits)
        if q is None:
            return None
        out.append(q)
    return out


def model_rows_ok(model, codes):
    rows = model[sorted(set(codes))].astype(np.int64)
    return bool(((rows[:, 1] >= 1) & (np.abs(rows[:, 0]) < Q_LIMIT) & (np.abs(rows[:, 2]) < OFFSET_LIMIT)).all())


def align_read(q, codes, model, S, max_cost, W):
    """q: T quantised samples; codes: the k-mer of each of the N states, 1 <= N <= T; W: the band, or None for no band.
    Returns (score, states [T]) of the minimum-cost path inside the band, ties as the definition says."""
    T, N = len(q), len(codes)
    if W is None:
        W = N
    rows = model[np.asarray(codes, dtype=np.int64)]
    level, weight, offset = rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy()
    cost = np.full(N + 1, INF, dtype=np.int64)                       # cost[1 + j]: state j at the previous sample; cost[0] stays INF
    back = np.zeros((T, W), dtype=bool)                              # back[t, j - lo(t)]: state j at t came by a step
    plo = 0
    for t in range(T):
        lo = band_lo(t, N, T, W)
        hi = min(lo + W, N)
        if t == 0:
            assert lo == 0
            new = np.full(hi, INF, dtype=np.int64)
            new[0] = 0
            took = np.zeros(hi, dtype=bool)
        else:
            stay, step = cost[1 + lo:1 + hi], cost[lo:hi]            # outside the previous band both hold INF
            took = step < stay                                       # the step replaces the stay only if strictly smaller
            new = np.where(took, step, stay)
        live = new < INF
        new = np.where(live, new + cost_row(q[t], level[lo:hi], weight[lo:hi], offset[lo:hi], S, max_cost), INF)
        cost[1 + plo:1 + lo] = INF                                   # the states that left the band
        cost[1 + lo:1 + hi] = new
        back[t, :hi - lo] = took
        plo = lo
    score = int(cost[N])
    assert score < INF
    states = np.empty(T, dtype=np.int32)
    s = N - 1
    for t in range(T - 1, -1, -1):
        states[t] = s
        if back[t, s - band_lo(t, N, T, W)]:
            s -= 1
    assert s == 0
    return score, states


def band_hits_of(states, N, W):
    T = len(states)
    hits = 0
    for t, s in enumerate(states.tolist()):
        lo = band_lo(t, N, T, W)
        if (s == lo and lo > 0) or (s == lo + W - 1 and lo + W < N):
            hits += 1
    return hits


def starts_of(states, N, T, max_events):
    starts = np.full(max_events + 1, T, dtype=np.int32)
    s = np.asarray(states)
    first = np.flatnonzero(np.diff(s, prepend=-1) != 0)
    assert len(first) == N
    starts[:N] = first
    return starts


def signal_align_ref(signal, signal_lengths, labels, label_lengths, model, k=5, first=0, frac_bits=12, weight_shift=32, max_cost=None,
                     band=512, scale_shift=None, max_events=None):
    """signal [B, L] float32 or int16; labels [B, n]; model [4^k, 3] integers.  band=None: no band.  Returns a dict: starts
    [B, max_events + 1] int32, score [B] object (Python integers), band_hits [B] int32, states [B, L] int32, bad."""
    B, L = signal.shape
    n_lab = labels.shape[1]
    model = np.asarray(model, dtype=np.int64)
    max_cost = (1 << 31) - 1 if max_cost is None else int(max_cost)
    if max_events is None:
        max_events = max(n_lab - (k - 1) - 2 * first, 1)
    starts = np.full((B, max_events + 1), -1, dtype=np.int32)
    states = np.full((B, L), -1, dtype=np.int32)
    score, hits, bad = [BAD_READ] * B, np.full(B, -1, dtype=np.int32), 0
    for b in range(B):
        T, ll = int(signal_lengths[b]), int(label_lengths[b])
        N = ll - (k - 1) - 2 * first
        if not (0 <= T <= L and 0 <= ll <= n_lab and N <= max_events):
            bad += 1
            continue
        if N < 1 or T < N:
            score[b], hits[b] = NO_ALIGNMENT, 0
            continue
        codes = read_states(labels[b], ll, k, first)
        q = read_samples(signal[b], T, None if scale_shift is None else scale_shift[b], frac_bits)
        if codes is None or q is None or not model_rows_ok(model, codes):
            bad += 1
            continue
        sc, st = align_read(q, codes, model, weight_shift, max_cost, band)
        score[b] = sc
        hits[b] = 0 if band is None else band_hits_of(st, N, band)
        states[b, :T] = st
        starts[b] = starts_of(st, N, T, max_events)
    return {"starts": starts, "score": np.array(score, dtype=object), "band_hits": hits, "states": states, "bad": bad}


def rescore(q, codes, model, S, max_cost, starts):
    """the cost of the segmentation state j = samples [starts[j], starts[j + 1]) -- any segmentation, in Python integers"""
    model = np.asarray(model, dtype=np.int64)
    total = 0
    for j, code in enumerate(codes):
        level, weight, offset = (int(v) for v in model[code])
        for t in range(int(starts[j]), int(starts[j + 1])):
            total += sample_cost(q[t], level, weight, offset, S, max_cost)
    return total
