"""The definition of wn_event_detect (include/wavenet_amd.h) in Python integers: Welch's t^2 between two
equal windows as the rational A / V, compared exactly by cross-multiplication; a peak is the arg-max of its +-r neighbourhood,
ties to the smaller index; short peaks, long peaks without a short one within +-w_long, forced splits of long events.  Nothing
here is a float except the sample that is quantised.  `peaks_of` takes the two comparisons of the peak rule as arguments, so that
a test can swap them; `compare_log` records the operands of every comparison for the tests of the comparator's width."""
import collections

import numpy as np

from tests.signal_align_ref import read_samples

Detector = collections.namedtuple("Detector", "window radius threshold vmin")        # threshold: theta, on t^2 in units of 2^-8
MAX_WINDOW, MAX_RADIUS, MAX_VMIN, MAX_EVENT_LEN = 16, 64, 1 << 55, 65536
KIND_START, KIND_SHORT, KIND_LONG, KIND_FORCED = 0, 1, 2, 3


def theta_of(t):
    return max(1, int(round(t * t * 256)))


def vmin_of(min_var, frac_bits, window):
    return max(1, int(round(min_var * 4 ** frac_bits * window * window)))


def detectors(windows=(3, 6), thresholds=(4.0, 6.0), radii=None, min_var=0.01, frac_bits=12):
    """the two Detector tuples as wavenet_speech_amd.detect_events forms them"""
    radii = windows if radii is None else radii
    return tuple(Detector(w, max(r, 1), theta_of(t), vmin_of(min_var, frac_bits, max(w, 1))) for w, r, t in zip(windows, radii, thresholds))


def scores(q, det):
    """[(A_i, V_i)] for i in 0..T: the score of position i is A_i / V_i; (0, 1) outside [w, T - w]"""
    T, w = len(q), det.window
    out = [(0, 1)] * (T + 1)
    for i in range(w, T - w + 1):
        s1, s2 = sum(q[i - w:i]), sum(q[i:i + w])
        qq = sum(v * v for v in q[i - w:i + w])
        out[i] = (w * (s2 - s1) ** 2, max(w * qq - s1 * s1 - s2 * s2, det.vmin))
    return out


def passes(av, det):
    return av[0] * 256 >= det.threshold * av[1]


def peaks_of(sc, det, left=lambda x, y: x > y, right=lambda x, y: x >= y, compare_log=None):
    """the peaks of one detector: i passes the threshold, beats every j < i within r strictly and every j > i within r or ties"""
    n, r = len(sc), det.radius
    out = []
    for i in range(n):
        if not passes(sc[i], det):
            continue
        ok = True
        for j in range(max(i - r, 0), min(i + r, n - 1) + 1):
            if j == i:
                continue
            x, y = sc[i][0] * sc[j][1], sc[j][0] * sc[i][1]
            if compare_log is not None:
                compare_log.append((x, y))
            if not (left(x, y) if j < i else right(x, y)):
                ok = False
                break
        if ok:
            out.append(i)
    return out


def boundaries_of(q, dets, max_event_len=MAX_EVENT_LEN, **how):
    """[(position, kind)] of a read of T >= 1 quantised samples, forced splits included"""
    T = len(q)
    short = peaks_of(scores(q, dets[0]), dets[0], **how)
    marks = {0: KIND_START}
    for p in short:
        marks[p] = KIND_SHORT
    if dets[1].window > 0:
        w1 = dets[1].window
        for p in peaks_of(scores(q, dets[1]), dets[1], **how):
            if not any(abs(p - s) <= w1 for s in short):
                marks[p] = KIND_LONG
    natural = sorted(marks)
    out = []
    for left, right in zip(natural, natural[1:] + [T]):
        out.append((left, marks[left]))
        out.extend((p, KIND_FORCED) for p in range(left + max_event_len, right, max_event_len))
    return out


def event_detect_ref(signal, signal_lengths, dets, frac_bits=12, max_event_len=MAX_EVENT_LEN, max_events=None, scale_shift=None, **how):
    """What wn_event_detect writes: a dict of n_events [B] int32, starts [B, N + 1] int32, sum / sumsq [B, N] (Python integers in
    object arrays), kind [B, N] int32 and bad (the count)"""
    signal = np.asarray(signal)
    if signal.ndim == 3:
        signal = signal[:, 0, :]
    B, L = signal.shape
    N = L if max_events is None else max_events
    n_events = np.zeros(B, dtype=np.int32)
    starts = np.zeros((B, N + 1), dtype=np.int32)
    ev_sum, ev_sumsq = np.zeros((B, N), dtype=object), np.zeros((B, N), dtype=object)
    kind = np.full((B, N), -1, dtype=np.int32)
    bad = 0
    for b in range(B):
        T = int(signal_lengths[b])
        q = read_samples(signal[b], T, None if scale_shift is None else scale_shift[b], frac_bits) if 0 <= T <= L else None
        if q is None:
            n_events[b], starts[b], bad = -1, -1, bad + 1
            continue
        bounds = boundaries_of(q, dets, max_event_len, **how) if T else []
        n_events[b] = len(bounds)
        starts[b] = T
        edges = [p for p, _ in bounds] + [T]
        for e, (p, kd) in enumerate(bounds[:N + 1]):
            starts[b, e] = p
            if e < N:
                seg = q[p:edges[e + 1]]
                ev_sum[b, e], ev_sumsq[b, e], kind[b, e] = sum(seg), sum(v * v for v in seg), kd
    return dict(n_events=n_events, starts=starts, sum=ev_sum, sumsq=ev_sumsq, kind=kind, bad=bad)
