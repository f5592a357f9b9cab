"""Inputs of the kmer_events tests, built once (seeded numpy), with their references from tests/kmer_events_ref.py cached per
(case, layout, signal kind, frac_bits).  A case is a set of reads with contiguous events (`starts`, as RaggedReads.starts) and
optional gaps cut off the end of each event; the two layouts of the Python interface read it as
    "starts"   event j = [starts[j], starts[j + 1]), every read has N events (the empty trailing ones get code -2)
    "spans"    event j = [starts[j], starts[j + 1] - gaps[j]), rows past label_lengths[b] are -1, every read has label_lengths[b] events
and the two signal kinds as float32 picoamps, or int16 raw = round(8 x) with a per-read float32 (scale, shift)."""
import collections
import functools

import numpy as np

from tests import kmer_events_ref as R
from tests.signal_align_cases import int16_of

Case = collections.namedtuple("Case", "signal signal_lengths labels label_lengths starts gaps kw")
LAYOUTS = ("spans", "starts")
KINDS = ("f32", "i16")


def _build(seed, dwell_rows, kw, label_extra=0, gaps=False, cut=None):
    """dwell_rows: per read the list of event lengths in FRAMES.  label_lengths = events + label_extra; the events past a read's
    own are empty."""
    rng = np.random.default_rng(seed)
    fs, fo = kw.get("frame_stride", 1), kw.get("frame_offset", 0)
    B, N = len(dwell_rows), max(len(r) for r in dwell_rows) + max(label_extra, 0)        # "spans" has one event per label
    starts = np.zeros((B, N + 1), dtype=np.int32)
    for b, row in enumerate(dwell_rows):
        c = np.concatenate([[0], np.cumsum(row)])
        starts[b, :len(c)] = c
        starts[b, len(c):] = c[-1]
    ends = starts[:, -1].astype(np.int64) * fs + fo
    L = int(ends.max()) + 3
    signal = (90.0 + 12.0 * rng.standard_normal((B, L))).astype(np.float32)
    signal_lengths = ends.astype(np.int32)
    if cut is not None:
        for b, n in cut.items():
            signal_lengths[b] = n
    n_events = np.array([len(r) for r in dwell_rows], dtype=np.int32)
    label_lengths = np.maximum(n_events + label_extra, 0).astype(np.int32)
    labels = rng.integers(1, 5, size=(B, max(int(label_lengths.max()), N, 1) + 2)).astype(np.int32)
    g = np.zeros((B, N), dtype=np.int32)
    if gaps:
        width = starts[:, 1:] - starts[:, :-1]
        g = np.minimum(rng.integers(0, 3, size=(B, N)), width).astype(np.int32)
    return Case(signal, signal_lengths, labels, label_lengths, starts, g, kw)


def _short(rng, n, lo=1, hi=10):
    return rng.integers(lo, hi, size=n).tolist()


def _cases():
    rng = np.random.default_rng(7)
    c = {}
    c["single_event"] = _build(1, [[5]], dict(k=1, first=0))
    c["wave_edges_65_129"] = _build(2, [_short(rng, 65), _short(rng, 129), _short(rng, 64)], dict(k=5, first=-2))
    mid = _short(rng, 70)
    mid[20], mid[41] = 64, 65
    with_max, over_max = _short(rng, 30), _short(rng, 30)
    with_max[9], over_max[13] = 65536, 65537
    c["long_events"] = _build(3, [mid, with_max, over_max, _short(rng, 12, 30, 40)], dict(k=5, first=-2))
    c["gaps"] = _build(4, [_short(rng, 40, 2, 9), _short(rng, 33, 1, 5)], dict(k=5, first=-2), gaps=True)
    c["frames_stride3_offset2"] = _build(5, [_short(rng, 70), _short(rng, 20)], dict(k=5, first=-2, frame_stride=3, frame_offset=2))
    c["labels_shorter_than_k"] = _build(6, [_short(rng, 3), _short(rng, 4), _short(rng, 1)], dict(k=5, first=0))
    c["first_0"] = _build(7, [_short(rng, 30), _short(rng, 66)], dict(k=5, first=0), label_extra=4)
    c["first_plus2"] = _build(8, [_short(rng, 30), _short(rng, 66)], dict(k=5, first=2), label_extra=8)
    c["k1"] = _build(9, [_short(rng, 50), _short(rng, 10)], dict(k=1, first=0))
    c["k6"] = _build(10, [_short(rng, 300), _short(rng, 140)], dict(k=6, first=-2))
    c["max_dwell_1"] = _build(11, [_short(rng, 40, 1, 4), _short(rng, 9, 1, 4)], dict(k=2, first=0, max_dwell=1), label_extra=1)
    rows = [_short(rng, 14, 3, 8), _short(rng, 14, 3, 8)]
    edge = int(np.cumsum(rows[0])[9]) + 1                          # inside event 10 of read 0: it is cut, 11.. lie wholly past
    c["cut_by_signal_length"] = _build(12, rows, dict(k=3, first=-1), cut={0: edge, 1: 0})
    return c


CASES = _cases()


def segments(case, layout):
    """(begin, end, events) of a case under a layout, [B, N] int32 and [B] int32"""
    B, N = case.gaps.shape
    if layout == "starts":
        return case.starts[:, :-1].copy(), case.starts[:, 1:].copy(), np.full(B, N, dtype=np.int32)
    spans = spans_of(case)
    return spans[:, :, 0].copy(), spans[:, :, 1].copy(), case.label_lengths.copy()


def spans_of(case):
    B, N = case.gaps.shape
    spans = np.stack([case.starts[:, :-1], case.starts[:, 1:] - case.gaps], axis=2).astype(np.int32)
    spans[np.arange(N)[None, :] >= case.label_lengths[:, None]] = -1
    return spans


@functools.lru_cache(maxsize=None)
def int16_form(name):
    return int16_of(CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name, layout, kind, frac_bits):
    case = CASES[name]
    begin, end, events = segments(case, layout)
    signal, ss = (case.signal, None) if kind == "f32" else int16_form(name)
    return R.kmer_events_ref(signal, case.signal_lengths, case.labels, case.label_lengths, begin, end, events, scale_shift=ss,
                             frac_bits=frac_bits, **dict(dict(max_dwell=255), **case.kw))


# ---- bad reads mixed into a batch of good ones: 20 events of 2..6 samples each, k = 5, first = -2, frac_bits = 12
BAD_KW = dict(k=5, first=-2, max_dwell=255)
BAD_READS = ("good", "overlap_or_reversed", "reversed", "negative_boundary", "label_0", "label_5", "nan_used", "inf_used", "range_used",
             "poison_in_skipped_events", "good_again", "signal_length_above", "signal_length_negative", "label_length_above",
             "label_length_negative")


@functools.lru_cache(maxsize=None)
def bad_batch():
    rng = np.random.default_rng(21)
    case = _build(20, [_short(rng, 20, 2, 7) for _ in BAD_READS], BAD_KW)
    signal, labels = case.signal.copy(), case.labels[:, :20].copy()                # labels exactly as wide as the events
    sl, ll, st = case.signal_lengths.copy(), case.label_lengths.copy(), case.starts
    r = BAD_READS.index
    labels[r("label_0"), 7] = 0
    labels[r("label_5"), 19] = 5                                      # the last label: in the window of event 17 only
    signal[r("nan_used"), st[r("nan_used"), 9]] = np.nan
    signal[r("inf_used"), st[r("inf_used"), 3] - 1] = -np.inf           # the last sample of event 2, the first used one
    signal[r("range_used"), st[r("range_used"), 18] - 1] = 2048.0       # 2048 * 2^12 = 2^23: the first value out of range
    p = r("poison_in_skipped_events")                                 # events 0, 1, 18, 19 have code -1 with first = -2, k = 5
    signal[p, st[p, 0]] = np.nan
    signal[p, st[p, 2] - 1] = np.inf
    signal[p, st[p, 18]] = 1e30
    signal[p, st[p, 20]:] = np.nan                                    # and past the read
    signal[r("good_again"), st[r("good_again"), 5]] = 2047.99         # the in-range side of the limit
    sl[r("signal_length_above")] = signal.shape[1] + 1
    sl[r("signal_length_negative")] = -1
    ll[r("label_length_above")] = labels.shape[1] + 1
    ll[r("label_length_negative")] = -1
    return Case(signal, sl, labels, ll, st, case.gaps, BAD_KW)


def bad_segments(layout):
    """(seg array for the interface, begin, end, events): spans [B, N, 2] or starts [B, N + 1] with the boundary faults put in"""
    case = bad_batch()
    r = BAD_READS.index
    B, N = case.gaps.shape
    if layout == "spans":
        seg = np.stack([case.starts[:, :-1], case.starts[:, 1:]], axis=2).astype(np.int32)
        seg[r("overlap_or_reversed"), 5, 0] -= 1                      # begins inside event 4
        seg[r("reversed"), 7, 1] = seg[r("reversed"), 7, 0] - 1
        seg[r("negative_boundary"), 0, 0] = -1
        return seg, seg[:, :, 0].copy(), seg[:, :, 1].copy(), case.label_lengths.copy()
    seg = case.starts.copy()
    seg[r("overlap_or_reversed"), 5] = seg[r("overlap_or_reversed"), 6] + 1          # event 5 ends before it begins
    seg[r("reversed"), 20] = seg[r("reversed"), 19] - 1
    seg[r("negative_boundary"), 0] = -1
    return seg, seg[:, :-1].copy(), seg[:, 1:].copy(), np.full(B, N, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def bad_reference(layout):
    case = bad_batch()
    _, begin, end, events = bad_segments(layout)
    return R.kmer_events_ref(case.signal, case.signal_lengths, case.labels, case.label_lengths, begin, end, events, frac_bits=12,
                             **BAD_KW)


def bad_expected(layout):
    """per read of BAD_READS, whether it must come out bad (the same under both layouts)"""
    good = {"good", "poison_in_skipped_events", "good_again"}
    return [name not in good for name in BAD_READS]
