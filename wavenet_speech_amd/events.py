"""
Event tables and k-mer pore-model fitting from alignments (csrc/wn_events.hip through the C ABI's
wn_kmer_events).

    reads = ragged_reads(64, (200, 300), device="cuda")                                   # or real signal + ctc_forced_align spans
    ev = kmer_events(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, starts=reads.starts, first=2)
    means, stdvs, counts = fit_kmer_model(ev.kmer_stats, prior=standin_kmer_table())
    dwell = fit_dwell_model(ev.dwell_hist, sample_rate=4000.0)                            # ("gamma", shape, rate, sample_rate)
    again = ragged_reads(64, (200, 300), table=(means, stdvs), dwell=dwell, device="cuda")

What the reference does off-line from nanopolish `eventalign` files (utils/dump_distributions.py: samples per k-mer;
utils/dump_durations_from_eventalign.py: a gamma dwell model per 5-mer), from signal that is on the device already.  kmer_events
is HIP only (no CPU fallback); the fits and the text formatter run on the host on the small tables.

Where no segmentation exists yet, signal_align (csrc/wn_sigalign.hip through wn_signal_align) makes one from
the signal, the known bases and a table alone -- what nanopolish does before `eventalign` prints anything -- and the loop
align -> kmer_events -> fit_kmer_model -> align again is Viterbi training of the table:

    model = signal_model(*standin_kmer_table())                                            # or a fitted (means, stdvs)
    al = signal_align(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, model, first=2, band=128)
    ev = kmer_events(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, starts=al.starts, k=al.k, first=al.first)
    model = signal_model(*fit_kmer_model(ev.kmer_stats, prior=standin_kmer_table())[:2])

Where not even the bases exist, detect_events (csrc/wn_eventdetect.hip through wn_event_detect) cuts a bare read
into events -- where its level changes, by Welch's t^2 at two window lengths -- and its event means are a shorter read for
mapping.signal_map and signal_align:

    found = detect_events(signal, signal_lengths, max_events=4096)                         # n_events, starts, sum, sumsq, kind
    means, counts = found.as_signal()
    hit = signal_map(means, counts, map_reference(lambda_bases, model))                    # 4096 events instead of 4096 samples

On noisy reads the detector misses boundaries, so a read has fewer events than k-mers and signal_align, which never skips, has no
alignment for it.  event_align (csrc/wn_eventalign.hip through wn_event_align) aligns the events themselves --
stay, step, or skip one or two k-mers, an event's cost weighing its length -- and its starts, in samples, go into kmer_events:

    al = event_align(found, bases, base_lengths, model, first=2)                           # EventAlignment: starts, score, moves
    ev = kmer_events(signal, signal_lengths, bases, base_lengths, starts=al.starts, k=al.k, first=al.first)
    al = event_align(found, bases, base_lengths, model, first=2, moves=fit_moves(al.moves))
"""
import math
from collections import namedtuple
from fractions import Fraction

import torch

from . import _args, _lib
from ._args import _alloc_bytes, _p, _stream
from .decoding import DEFAULT_ALPHABET

MAX_K = 6
MAX_FIRST = 8
MAX_FRAC_BITS = 20
MAX_DWELL = 65536
MIN_WEIGHT_SHIFT, MAX_WEIGHT_SHIFT = 16, 63
MIN_BAND, MAX_BAND = 64, 2048
MAX_ALIGN_SIGNAL = 1 << 24
MAX_ALIGN_EVENTS = 1 << 20
EVENTALIGN_COLUMNS = ("read_index", "position", "reference_kmer", "event_index", "event_level_mean", "event_stdv", "event_length",
                      "event_start_time", "model_mean", "model_stdv", "standardized_level")

_Fields = namedtuple("KmerEvents", "kmer start length sum sumsq read_counts kmer_stats dwell_hist")


class KmerEvents(_Fields):
    """kmer [B, N] int32: the k-mer index of a used event, else -1 (its window runs off the labels), -2 (no samples), -3 (cut by
    the read's end, or above 65536 samples), -4 (bad read, or past the read's events); start, length [B, N] int32: the clipped
    sample range; sum, sumsq [B, N] int64: the sums of q = round(v 2^frac_bits) and of q^2 over a used event (0 elsewhere) -- the
    five are None with want_events=False; read_counts [B, 4] int32: events used, with code -1, with code -2 or -3, samples used
    (-1 throughout for a bad read); kmer_stats [4^k, 5] int64: events, samples, sum q, and the low and high 32-bit limbs of
    sum q^2; dwell_hist [4^k, max_dwell + 1] int64: events by min(length, max_dwell).  Device tensors.  k, first, frac_bits and
    max_dwell of the call ride along as attributes."""

    def __new__(cls, *fields, k=5, first=-2, frac_bits=12, max_dwell=255):
        self = super().__new__(cls, *fields)
        self.k, self.first, self.frac_bits, self.max_dwell = int(k), int(first), int(frac_bits), int(max_dwell)
        return self

    @property
    def mean(self):
        """[B, N] float64: the level of every used event in the units of v, NaN elsewhere (one division of exact integers)"""
        n = torch.where(self.kmer >= 0, self.length, torch.zeros_like(self.length)).double()
        return self.sum.double() / (n * float(1 << self.frac_bits))          # 0 / 0 = NaN where the event is not used

    @property
    def stdv(self):
        """[B, N] float64: the population standard deviation of every used event, NaN elsewhere.  Formed as sumsq / n - (sum / n)^2
        in float64: its absolute error is about 2^-52 level^2 / stdv"""
        n = torch.where(self.kmer >= 0, self.length, torch.zeros_like(self.length)).double()
        m = self.sum.double() / n
        var = (self.sumsq.double() / n - m * m).clamp_(min=0.0)
        return var.sqrt() / float(1 << self.frac_bits)


def _read_inputs(what, signal, signal_lengths, labels, label_lengths, scale_shift):
    """what kmer_events and signal_align take alike: the signal as [B, L] rows and the int32 label rows, both read in place by
    their row stride, the two [B] length vectors and the [B, 2] scale_shift pair on the signal's device; then B, L and the device"""
    signal = _args.signal_rows(signal, what)
    dev = signal.device
    B, L = int(signal.shape[0]), int(signal.shape[1])
    labels = _args.int_rows(labels, what, "labels", B=B, shape="(%d, n >= 1)" % B, min_width=1, device=dev)
    with torch.cuda.device(dev):
        signal_lengths = _args.lengths(signal_lengths, B, dev, what, "signal_lengths", flatten=True)
        label_lengths = _args.lengths(label_lengths, B, dev, what, "label_lengths", flatten=True)
        scale_shift = _args.scale_shift(scale_shift, B, dev, what)
    return signal, signal_lengths, labels, label_lengths, scale_shift, B, L, dev


def kmer_events(signal, signal_lengths, labels, label_lengths, spans=None, starts=None, k=5, first=-2, frame_stride=1,
                frame_offset=0, scale_shift=None, frac_bits=12, max_dwell=255, into=None, want_events=True):
    """The event table of a segmentation and the k-mer tables a pore model is fitted from.

    signal          [B, L] or [B, 1, L], float32 or int16; a view is passed by its row stride (unit stride along L)
    signal_lengths  [B]; labels [B, n] bases in 1..4 with label_lengths [B]
    spans           [B, N, 2] int32, CTCAlignment.spans: event j = base j over the frames [spans[b, j, 0], spans[b, j, 1]); each
                    read has label_lengths[b] events
    starts          [B, N + 1] int32, RaggedReads.starts: event j = [starts[b, j], starts[b, j + 1]); each read has N events, the
                    empty ones past a read's last k-mer get code -2.  Exactly one of spans / starts.
    k, first        the k-mer of event j is labels[j + first .. j + first + k), first base most significant as KMER_WEIGHTS; first =
                    -2: centred 5-mers over force-aligned bases; first = 2 / 0: the generator's "loader" / "generator" windows
    frame_stride, frame_offset   a boundary f stands for sample f * frame_stride + frame_offset (the stride and the receptive
                    field's offset of the network the frames came from)
    scale_shift     [B, 2] float32 or None: v = x * scale + shift in float64 (from read_normalisation's pair: (scale, shift * scale))
    frac_bits, max_dwell   q = round(v * 2^frac_bits), |q| < 2^23; the dwell histogram has max_dwell + 1 columns, the last one
                    holds everything at or above max_dwell
    into            an earlier KmerEvents whose two tables are accumulated in place (and returned); per-read fields are replaced
    want_events     False: only read_counts and the tables are produced
    Integer arithmetic, bitwise reproducible, no host synchronisation (capturable with fixed shapes).  A bad read (lengths out of
    range, negative / reversed / overlapping boundaries, a label outside 1..4 or a non-finite or out-of-range sample in a used
    event) has kmer -4, zeros elsewhere, read_counts -1, adds nothing to the tables and is reported through
    check_device_flags().  Returns KmerEvents."""
    what = "kmer_events"
    signal, signal_lengths, labels, label_lengths, scale_shift, B, L, dev = _read_inputs(what, signal, signal_lengths, labels,
                                                                                         label_lengths, scale_shift)
    if (spans is None) == (starts is None):
        raise ValueError("wavenet_speech_amd.%s: give exactly one of spans and starts" % what)
    k, first, F, D = int(k), int(first), int(frac_bits), int(max_dwell)
    if not 1 <= k <= MAX_K or abs(first) > MAX_FIRST or not 0 <= F <= MAX_FRAC_BITS or not 1 <= D <= MAX_DWELL:
        raise ValueError("wavenet_speech_amd.%s: k in [1, %d], |first| <= %d, frac_bits in [0, %d], max_dwell in [1, %d]"
                         % (what, MAX_K, MAX_FIRST, MAX_FRAC_BITS, MAX_DWELL))
    frame_stride, frame_offset = int(frame_stride), int(frame_offset)
    if frame_stride < 1 or frame_offset < 0 or L * frame_stride >= 2 ** 31:
        raise ValueError("wavenet_speech_amd.%s: frame_stride >= 1, frame_offset >= 0 and L * frame_stride < 2^31" % what)
    with torch.cuda.device(dev):
        if spans is not None:
            seg = _args.gpu_tensor(spans, what, "spans", (torch.int32,), ValueError, dev)
            if seg.dim() != 3 or seg.shape[0] != B or seg.shape[1] < 1 or seg.shape[2] != 2:
                raise ValueError("wavenet_speech_amd.%s: spans must be [%d, N >= 1, 2], got %s" % (what, B, tuple(seg.shape)))
            if seg.stride(2) != 1 or seg.stride(0) < 0 or seg.stride(1) < 0:
                seg = seg.contiguous()
            N, end_offset, events = int(seg.shape[1]), 1, label_lengths
        else:
            seg = _args.gpu_tensor(starts, what, "starts", (torch.int32,), ValueError, dev)
            if seg.dim() != 2 or seg.shape[0] != B or seg.shape[1] < 2:
                raise ValueError("wavenet_speech_amd.%s: starts must be [%d, N + 1 >= 2], got %s" % (what, B, tuple(seg.shape)))
            if seg.stride(0) < 0 or seg.stride(1) < 0:
                seg = seg.contiguous()
            N, end_offset = int(seg.shape[1]) - 1, int(seg.stride(1))
            events = torch.full((B,), N, dtype=torch.int32, device=dev)
        if into is not None and not isinstance(into, KmerEvents):
            raise ValueError("wavenet_speech_amd.%s: into must be a KmerEvents, got %s" % (what, type(into).__name__))
        if into is not None and (into.k, into.first, into.frac_bits, into.max_dwell) != (k, first, F, D):
            raise ValueError("wavenet_speech_amd.%s: into was made with other k, first, frac_bits or max_dwell" % what)
        lib = _lib.load()
        kmer_stats = _args.into_table(into, "kmer_stats", (4 ** k, 5), dev, what)
        dwell_hist = _args.into_table(into, "dwell_hist", (4 ** k, D + 1), dev, what)
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        ev = [None] * 5
        if want_events:
            ev = [torch.empty(B, N, **i32) for _ in range(3)] + [torch.empty(B, N, **i64) for _ in range(2)]
        read_counts = torch.empty(B, 4, **i32)
        bad = torch.zeros(1, **i32)
        ws = _alloc_bytes(lib.wn_kmer_events_workspace_bytes(B, N), "wn_kmer_events_workspace_bytes", dev, status=-2)
        seg_end = seg.data_ptr() + 4 * end_offset
        _lib.check(lib.wn_kmer_events(_p(signal), int(signal.dtype == torch.int16), signal.stride(0), _p(signal_lengths), _p(scale_shift),
                                      _p(seg), _p(seg_end), seg.stride(0), seg.stride(1), frame_stride, frame_offset, _p(labels),
                                      labels.stride(0), _p(label_lengths), _p(events), B, L, int(labels.shape[1]), N, k, first, F, D,
                                      _p(ev[0]), _p(ev[1]), _p(ev[2]), _p(ev[3]), _p(ev[4]), _p(read_counts), _p(kmer_stats),
                                      _p(dwell_hist), _p(ws), ws.numel(), _p(bad), _stream()), "wn_kmer_events")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.kmer_events: %d bad read(s): a length out of range, a negative, reversed or "
                       "overlapping event boundary, a label outside 1..4 or a non-finite or out-of-range sample in a used event" % n)
    return KmerEvents(ev[0], ev[1], ev[2], ev[3], ev[4], read_counts, kmer_stats, dwell_hist, k=k, first=first, frac_bits=F, max_dwell=D)


def _host_table(t, what, name, columns=None):
    rows = torch.as_tensor(t)
    if rows.is_floating_point() or rows.dim() != 2 or (columns is not None and rows.shape[1] != columns):
        raise ValueError("wavenet_speech_amd.%s: %s must be a 2-d integer table%s" % (what, name, "" if columns is None else " with %d columns" % columns))
    return rows.cpu().tolist()


def fit_kmer_model(kmer_stats, frac_bits=12, min_count=100, prior=None):
    """The pore model of a kmer_stats table ([4^k, 5] integers): returns (means, stdvs, counts), float64 [4^k] host tensors --
    what ragged_reads(table=...) and RawGaussianModelLoader take.  Per k-mer with n samples, S1 = sum q and S2 = high limb * 2^32
    + low limb = sum q^2: mean = S1 / (n 2^F), stdv = sqrt((n S2 - S1^2) / (n^2 2^2F)), the POPULATION standard deviation of its
    samples.  Both numerators and denominators are exact Python integers divided once (correctly rounded), so mean carries one
    float64 rounding and stdv two.  counts: the samples of each k-mer.  A k-mer with fewer than min_count samples takes its
    entry of prior = (means, stdvs), or NaN.  Runs on the host: the table is 40 KB at k = 5."""
    what = "fit_kmer_model"
    rows = _host_table(kmer_stats, what, "kmer_stats", 5)
    F, min_count = int(frac_bits), int(min_count)
    if not 0 <= F <= MAX_FRAC_BITS or min_count < 1:
        raise ValueError("wavenet_speech_amd.%s: frac_bits in [0, %d] and min_count >= 1" % (what, MAX_FRAC_BITS))
    nan = float("nan")
    pm = ps = None
    if prior is not None:
        pm, ps = (torch.as_tensor(p).double().cpu().reshape(-1).tolist() for p in prior)
        if len(pm) != len(rows) or len(ps) != len(rows):
            raise ValueError("wavenet_speech_amd.%s: prior must hold %d means and stdvs" % (what, len(rows)))
    means, stdvs, counts = [], [], []
    for i, (_, n, s1, lo, hi) in enumerate(rows):
        counts.append(float(n))
        if n < min_count:
            means.append(pm[i] if pm else nan)
            stdvs.append(ps[i] if ps else nan)
            continue
        s2 = (hi << 32) + lo
        means.append(s1 / (n << F))
        stdvs.append(math.sqrt((n * s2 - s1 * s1) / ((n * n) << (2 * F))))
    f64 = dict(dtype=torch.float64)
    return torch.tensor(means, **f64), torch.tensor(stdvs, **f64), torch.tensor(counts, **f64)


def _digamma(x):
    return float(torch.special.digamma(torch.tensor(x, dtype=torch.float64)))


def _trigamma(x):
    return float(torch.special.polygamma(1, torch.tensor(x, dtype=torch.float64)))


def _gamma_shape(s):
    """the root a of log a - digamma(a) = s, s > 0: Minka's start and his Newton step on 1 / a, float64"""
    a = (3.0 - s + math.sqrt((s - 3.0) ** 2 + 24.0 * s)) / (12.0 * s)
    for _ in range(100):
        f = math.log(a) - _digamma(a) - s
        step = f / (a * a * (1.0 / a - _trigamma(a)))
        new = 1.0 / (1.0 / a + step)
        if not (new > 0.0 and math.isfinite(new)):
            break
        done = abs(new - a) <= 4e-16 * a
        a = new
        if done:
            break
    return a


def _fit_gamma(hist, sample_rate):
    """hist[d] events of d samples (hist[0] ignored) -> (shape, rate, events) of the maximum-likelihood gamma of d / sample_rate"""
    n = sum(hist[1:])
    mean_d = math.fsum(d * h for d, h in enumerate(hist) if d and h) / n
    mean_log = math.fsum(h * math.log(d) for d, h in enumerate(hist) if d and h) / n
    s = math.log(mean_d) - mean_log
    if not s > 1e-14:
        raise ValueError("wavenet_speech_amd.fit_dwell_model: every event has the same length: the gamma shape is unbounded")
    a = _gamma_shape(s)
    return a, a * sample_rate / mean_d, n


def fit_dwell_model(dwell_hist, sample_rate, per_kmer=False, min_count=100):
    """The gamma dwell model of a dwell_hist table ([4^k, D + 1] integers): the maximum-likelihood gamma of the event durations
    d / sample_rate seconds, as the reference's utils/dump_durations_from_eventalign.py fits per 5-mer.  The shape a solves
    log a - digamma(a) = log(mean d) - mean(log d) (Newton from Minka's closed-form start, float64); rate = a sample_rate / mean d.
    per_kmer=False: all k-mers pooled; returns ("gamma", shape, rate, sample_rate), the dwell spec of ragged_reads; raises below
    min_count events.  per_kmer=True: returns a float64 [4^k, 2] host tensor of (shape, rate), NaN for a k-mer with fewer than
    min_count events or with events of one length only.
    Raises if the last column, which holds every event of D samples or more, is not empty: rerun kmer_events with a larger
    max_dwell.  Dwells are whole samples: the generator truncates Gamma * sample_rate to an integer (and lifts 0 to 1), so a fit to
    its output is biased low in the mean by about half a sample -- as the reference script's fit to nanopolish's event lengths."""
    what = "fit_dwell_model"
    rows = _host_table(dwell_hist, what, "dwell_hist")
    sample_rate, min_count = float(sample_rate), int(min_count)
    if len(rows[0]) < 2 or not (sample_rate > 0 and math.isfinite(sample_rate)) or min_count < 1:
        raise ValueError("wavenet_speech_amd.%s: at least two columns, sample_rate > 0 and min_count >= 1" % what)
    clamped = sum(r[-1] for r in rows)
    if clamped:
        raise ValueError("wavenet_speech_amd.%s: %d event(s) in the clamp column (%d samples or more): use a larger max_dwell"
                         % (what, clamped, len(rows[0]) - 1))
    if not per_kmer:
        pooled = [sum(col) for col in zip(*rows)]
        if sum(pooled[1:]) < min_count:
            raise ValueError("wavenet_speech_amd.%s: %d event(s), fewer than min_count = %d" % (what, sum(pooled[1:]), min_count))
        a, rate, _ = _fit_gamma(pooled, sample_rate)
        return ("gamma", a, rate, sample_rate)
    out = []
    for r in rows:
        try:
            if sum(r[1:]) < min_count:
                raise ValueError
            a, rate, _ = _fit_gamma(r, sample_rate)
            out.append([a, rate])
        except ValueError:
            out.append([float("nan")] * 2)
    return torch.tensor(out, dtype=torch.float64)


def eventalign_rows(events, labels, names=None, model=None, alphabet=DEFAULT_ALPHABET, sample_rate=None, header=True):
    """host formatter: the event table as the tab-separated lines of nanopolish `eventalign`, with the columns this library can
    fill (EVENTALIGN_COLUMNS): read_index (names[b] when given, else b), position (of the k-mer's first base, j + first),
    reference_kmer (alphabet[label] per base), event_index j, event_level_mean (%.2f), event_stdv (%.3f), event_length and
    event_start_time (samples; seconds %.5f with sample_rate), and with model = (means, stdvs): model_mean, model_stdv (%.2f) and
    standardized_level (%.2f) = (level - model_mean) / model_stdv.  Events with a negative code are left out.  events: a
    KmerEvents with its per-event fields; labels: the labels it was made from.  Returns a list of lines without line ends."""
    if not isinstance(events, KmerEvents) or events.kmer is None:
        raise ValueError("eventalign_rows: events must be a KmerEvents with its per-event fields (want_events=True)")
    k, first = events.k, events.first
    kmer = events.kmer.cpu().tolist()
    start, length = events.start.cpu().tolist(), events.length.cpu().tolist()
    mean, stdv = events.mean.cpu().tolist(), events.stdv.cpu().tolist()
    rows = torch.as_tensor(labels).cpu().tolist()
    if len(rows) != len(kmer) or (names is not None and len(names) != len(kmer)):
        raise ValueError("eventalign_rows: %d reads, %d label rows, %s names" % (len(kmer), len(rows), "no" if names is None else len(names)))
    mm = ms = None
    if model is not None:
        mm, ms = (torch.as_tensor(p).double().cpu().reshape(-1).tolist() for p in model)
    out = []
    if header:
        out.append("\t".join(EVENTALIGN_COLUMNS if model is not None else EVENTALIGN_COLUMNS[:8]))
    for b, codes in enumerate(kmer):
        name = str(names[b]) if names is not None else str(b)
        for j, code in enumerate(codes):
            if code < 0:
                continue
            text = "".join(alphabet[int(v)] for v in rows[b][j + first:j + first + k])
            if sample_rate is None:
                span = ["%d" % length[b][j], "%d" % start[b][j]]
            else:
                span = ["%.5f" % (length[b][j] / float(sample_rate)), "%.5f" % (start[b][j] / float(sample_rate))]
            cols = [name, "%d" % (j + first), text, "%d" % j, "%.2f" % mean[b][j], "%.3f" % stdv[b][j]] + span
            if model is not None:
                cols += ["%.2f" % mm[code], "%.2f" % ms[code], "%.2f" % ((mean[b][j] - mm[code]) / ms[code])]
            out.append("\t".join(cols))
    return out


class SignalModel:
    """The integer pore model signal_align works under.  table: [4^k, 3] int32 host tensor, per k-mer
        level   the current in units of 2^-frac_bits (the units of the quantised samples q), |level| < 2^23
        weight  in [1, 2^31): a sample costs min((q - level)^2 weight >> weight_shift, max_cost) + offset
        offset  |offset| < 2^30
    Any table within these ranges may be filled by hand: SignalModel(table, weight_shift, frac_bits, cost_bits); cost_bits only
    scales SignalAlignment.nats (a cost of 2^cost_bits is one nat).  signal_model() fills it with -log N(v; mean, stdv)."""

    def __init__(self, table, weight_shift, frac_bits=12, cost_bits=8):
        what = "SignalModel"
        table = torch.as_tensor(table)
        if table.is_floating_point() or table.dim() != 2 or table.shape[1] != 3:
            raise ValueError("wavenet_speech_amd.%s: table must be [4^k, 3] integers, got %s %s" % (what, table.dtype, tuple(table.shape)))
        k = next((k for k in range(1, MAX_K + 1) if 4 ** k == table.shape[0]), None)
        if k is None:
            raise ValueError("wavenet_speech_amd.%s: table must have 4^k rows, k in [1, %d], got %d" % (what, MAX_K, table.shape[0]))
        table = table.detach().cpu().long()
        level, weight, offset = table[:, 0], table[:, 1], table[:, 2]
        if bool((level.abs() >= 2 ** 23).any()) or bool((weight < 1).any()) or bool((weight >= 2 ** 31).any()) or bool((offset.abs() >= 2 ** 30).any()):
            raise ValueError("wavenet_speech_amd.%s: |level| < 2^23, weight in [1, 2^31) and |offset| < 2^30" % what)
        self.weight_shift, self.frac_bits, self.cost_bits, self.k = int(weight_shift), int(frac_bits), int(cost_bits), k
        if not MIN_WEIGHT_SHIFT <= self.weight_shift <= MAX_WEIGHT_SHIFT or not 0 <= self.frac_bits <= MAX_FRAC_BITS or not 0 <= self.cost_bits <= 16:
            raise ValueError("wavenet_speech_amd.%s: weight_shift in [%d, %d], frac_bits in [0, %d], cost_bits in [0, 16]"
                             % (what, MIN_WEIGHT_SHIFT, MAX_WEIGHT_SHIFT, MAX_FRAC_BITS))
        self.table = table.int().contiguous()
        self._on = {}

    def on(self, device):
        """the table on a device (uploaded once per device, so that a later call can be captured into a graph)"""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = self.table.to(device)
        return self._on[device]


def signal_model(means, stdvs, frac_bits=12, cost_bits=8):
    """The SignalModel of a Gaussian pore model: the cost of a sample v in a k-mer is -log N(v; mean, stdv) in units of 2^-cost_bits
    nats, up to the constant log sqrt(2 pi) - frac_bits log 2 that every path shares.  means, stdvs: [4^k] floats -- what
    fit_kmer_model returns (with a prior, so that no entry is NaN) and what standin_kmer_table() gives.  With s = stdv 2^F exactly:
        level  = round(mean 2^F)                         (ties to even, as everywhere below)
        weight = round(2^(S + cost_bits) / (2 s^2))      so that d^2 weight >> S = 2^cost_bits d^2 / (2 s^2)
        offset = round(2^cost_bits ln s)                 (one float64 logarithm)
    S is the largest weight_shift in [16, 63] at which the largest weight (of the smallest stdv) stays below 2^31: it then lies in
    [2^30, 2^31) unless S = 63 came first.  Refused: a non-finite mean or stdv, a stdv <= 0, a level at or beyond 2^23, a largest
    weight that does not fit at S = 16, a smallest weight that rounds below 1 (the stdvs span more than the 31 bits hold)."""
    what = "signal_model"
    mm = torch.as_tensor(means, dtype=torch.float64).cpu().reshape(-1).tolist()        # a list of Python floats keeps its 53 bits
    ss = torch.as_tensor(stdvs, dtype=torch.float64).cpu().reshape(-1).tolist()
    F, cb = int(frac_bits), int(cost_bits)
    if len(mm) != len(ss) or len(mm) not in [4 ** k for k in range(1, MAX_K + 1)]:
        raise ValueError("wavenet_speech_amd.%s: means and stdvs must both hold 4^k entries, k in [1, %d]" % (what, MAX_K))
    if not 0 <= F <= MAX_FRAC_BITS or not 0 <= cb <= 16:
        raise ValueError("wavenet_speech_amd.%s: frac_bits in [0, %d], cost_bits in [0, 16]" % (what, MAX_FRAC_BITS))
    if not all(math.isfinite(m) for m in mm) or not all(math.isfinite(s) and s > 0 for s in ss):
        raise ValueError("wavenet_speech_amd.%s: every mean must be finite and every stdv finite and positive "
                         "(fit_kmer_model leaves NaN where a k-mer has no data: give it a prior)" % what)
    sq = [Fraction(s) * (1 << F) for s in ss]                         # stdv 2^F, exact
    smallest = min(sq)
    S = next((S for S in range(MAX_WEIGHT_SHIFT, MIN_WEIGHT_SHIFT - 1, -1)
              if round(Fraction(1 << (S + cb)) / (2 * smallest * smallest)) < 2 ** 31), None)
    if S is None:
        raise ValueError("wavenet_speech_amd.%s: the smallest stdv (%g) is too small for frac_bits = %d" % (what, min(ss), F))
    rows = []
    for m, s in zip(mm, sq):
        level = round(Fraction(m) * (1 << F))
        weight = round(Fraction(1 << (S + cb)) / (2 * s * s))
        if abs(level) >= 2 ** 23 or weight < 1:
            raise ValueError("wavenet_speech_amd.%s: a level at or beyond 2^23 or a weight below 1 (mean %g, stdv %g, weight_shift %d)"
                             % (what, m, float(s) / (1 << F), S))
        rows.append([level, weight, round((1 << cb) * math.log(float(s)))])
    return SignalModel(torch.tensor(rows, dtype=torch.int64), S, F, cb)


class _Nats:
    @property
    def nats(self):
        """[B] float64: score / 2^cost_bits (+-inf-like sentinels stay huge: mask with score first)"""
        return self.score.double() / float(1 << self.cost_bits)


class _BandCall:
    """What a call of signal_align and of event_align share, raised in the caller's name: the checks of model, first, band and
    max_cost (and of the events' frac_bits against the model's, where there are events), the number of states, and the outputs
    that every banded alignment has."""

    def __init__(self, what, model, first, band, max_cost, events_frac_bits=None):
        if not isinstance(model, SignalModel):
            raise ValueError("wavenet_speech_amd.%s: model must be a SignalModel (signal_model(means, stdvs)), got %s" % (what, type(model).__name__))
        if events_frac_bits is not None and events_frac_bits != model.frac_bits:
            raise ValueError("wavenet_speech_amd.%s: the events have frac_bits %d and the model %d" % (what, events_frac_bits, model.frac_bits))
        first, band = int(first), int(band)
        max_cost = 2 ** 31 - 1 if max_cost is None else int(max_cost)
        if not 0 <= first <= MAX_FIRST or not MIN_BAND <= band <= MAX_BAND or band % 64 or not 1 <= max_cost <= 2 ** 31 - 1:
            raise ValueError("wavenet_speech_amd.%s: first in [0, %d], band a multiple of 64 in [%d, %d], max_cost in [1, 2^31 - 1]"
                             % (what, MAX_FIRST, MIN_BAND, MAX_BAND))
        self.k, self.first, self.band, self.max_cost = model.k, first, band, max_cost

    def states(self, labels):            # of a read that uses all of labels' columns, at least 1: the width of starts - 1
        return max(int(labels.shape[1]) - (self.k - 1) - 2 * self.first, 1)

    @staticmethod
    def outputs(B, N, dev):              # starts, score, band_hits, bad
        i32 = dict(dtype=torch.int32, device=dev)
        return torch.empty(B, N + 1, **i32), torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, **i32), torch.zeros(1, **i32)


_AlignFields = namedtuple("SignalAlignment", "starts score band_hits states")


class SignalAlignment(_Nats, _AlignFields):
    """starts [B, N + 1] int32: starts[b, j] is the first sample of state (k-mer) j, every entry past the read's last state is
    signal_lengths[b] -- RaggedReads.starts' convention, so it goes into kmer_events(starts=...) as it is; score [B] int64: the cost
    of the path, LLONG_MAX where there is no alignment (no state, or fewer samples than states) and LLONG_MIN for a bad read;
    band_hits [B] int32: the samples whose state lies on the band's edge while the band could still have been wider there -- above 0
    the band was too narrow for this read; states [B, L] int32 with want_states, else None: the state of every sample, -1 past the
    read.  No alignment: starts and states -1, band_hits 0; a bad read: everything -1.  Device tensors.  k, first, frac_bits,
    cost_bits and band of the call ride along as attributes."""

    def __new__(cls, *fields, k=5, first=0, frac_bits=12, cost_bits=8, band=512):
        self = super().__new__(cls, *fields)
        self.k, self.first, self.frac_bits, self.cost_bits, self.band = int(k), int(first), int(frac_bits), int(cost_bits), int(band)
        return self


def signal_align(signal, signal_lengths, labels, label_lengths, model, first=0, band=512, scale_shift=None, max_cost=None,
                 want_states=False):
    """Align raw samples to the k-mers of known bases under a SignalModel: the minimum-cost path in which
    every sample stays in its k-mer or steps to the next one (no skips: every k-mer holds at least one sample), inside a band of
    `band` k-mers around the diagonal.

    signal          [B, L] or [B, 1, L], float32 or int16; a view is passed by its row stride (unit stride along L)
    signal_lengths  [B]; labels [B, n] bases in 1..4 (int32 or int64) with label_lengths [B].  The event means of
                    detect_events(...).as_signal() go in as a shorter read: one row per event instead of one per sample
    model           a SignalModel (signal_model(means, stdvs), or filled by hand); its k and frac_bits are the call's
    first           read b has label_lengths[b] - (k - 1) - 2 first states, state j the k-mer labels[j + first .. j + first + k);
                    first = 2 / 0: the generator's "loader" / "generator" windows
    band            a multiple of 64 in [64, 2048]; state j is allowed at sample t iff lo(t) <= j < lo(t) + band, lo(t) =
                    clamp(((2 t + 1) N) // (2 T) - band / 2, 0, max(N - band, 0))
    scale_shift     [B, 2] float32 or None, as kmer_events
    max_cost        the clamp of a sample's quadratic term, in [1, 2^31 - 1] (None: 2^31 - 1): an outlier costs no more
    want_states     also return the state of every sample
    Integer arithmetic, ties to the stay, bitwise reproducible, no host synchronisation (capturable with fixed shapes once the
    model has been used on the device).  A bad read (a length out of range, a label of the used window outside 1..4, a non-finite
    or out-of-range sample before signal_lengths[b]) is reported through check_device_flags().  HIP only.  Returns
    SignalAlignment."""
    what = "signal_align"
    signal, signal_lengths, labels, label_lengths, scale_shift, B, L, dev = _read_inputs(what, signal, signal_lengths, labels,
                                                                                         label_lengths, scale_shift)
    call = _BandCall(what, model, first, band, max_cost)
    k, first, band, max_cost, N = call.k, call.first, call.band, call.max_cost, call.states(labels)
    if L > MAX_ALIGN_SIGNAL or N > MAX_ALIGN_EVENTS or B > 65535:
        raise ValueError("wavenet_speech_amd.%s: at most 2^24 samples and 2^20 k-mers per read and 65535 reads" % what)
    with torch.cuda.device(dev):
        lib = _lib.load()
        table = model.on(dev)
        starts, score, band_hits, bad = call.outputs(B, N, dev)
        states = torch.empty(B, L, dtype=torch.int32, device=dev) if want_states else None
        ws = _alloc_bytes(lib.wn_signal_align_workspace_bytes(B, L, band), "wn_signal_align_workspace_bytes", dev, status=-2)
        _lib.check(lib.wn_signal_align(_p(signal), int(signal.dtype == torch.int16), signal.stride(0), _p(signal_lengths), _p(scale_shift),
                                       _p(labels), labels.stride(0), _p(label_lengths), _p(table), B, L, int(labels.shape[1]), N, k, first,
                                       model.frac_bits, model.weight_shift, max_cost, band, _p(starts), _p(score), _p(band_hits),
                                       _p(states), _p(ws), ws.numel(), _p(bad), _stream()), "wn_signal_align")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.signal_align: %d bad read(s): a length out of range, a label outside 1..4, "
                       "a non-finite or out-of-range sample or a model row out of range" % n)
    return SignalAlignment(starts, score, band_hits, states, k=k, first=first, frac_bits=model.frac_bits, cost_bits=model.cost_bits,
                           band=band)


MAX_DETECT_WINDOW, MAX_DETECT_RADIUS, MAX_DETECT_VMIN, MAX_EVENT_LEN = 16, 64, 1 << 55, 65536
MAX_DETECT_SIGNAL = MAX_DETECT_EVENTS = 1 << 24
MIN_CHUNK, MAX_CHUNK = 256, 16384
DEFAULT_THRESHOLDS, DEFAULT_MIN_VAR = (4.0, 6.0), 0.01

_DetectFields = namedtuple("DetectedEvents", "n_events starts sum sumsq kind")


class DetectedEvents(_DetectFields):
    """n_events [B] int32: the events of each read -- the true count, even above max_events (the rows then hold the first
    max_events events whole), -1 for a bad read; starts [B, max_events + 1] int32: event e is the samples [starts[b, e],
    starts[b, e + 1]), every entry past the last event is signal_lengths[b] (SignalAlignment.starts' convention, so it goes into
    kmer_events(starts=...) as it is); sum, sumsq [B, max_events] int64: the sums of q = round(v 2^frac_bits) and of q^2 over the
    event, 0 past the last one; kind [B, max_events] int32: why the event begins -- 0 the read's start, 1 a peak of the short
    detector, 2 of the long one, 3 a forced split -- and -1 past the last event.  A bad read: starts -1, sums 0, kind -1.  Device
    tensors.  frac_bits and max_events of the call ride along as attributes."""

    def __new__(cls, *fields, frac_bits=12):
        self = super().__new__(cls, *fields)
        self.frac_bits, self.max_events = int(frac_bits), int(fields[2].shape[1])
        return self

    @property
    def held(self):
        """[B] int32: the events the rows hold, min(n_events, max_events); 0 for a bad read"""
        return self.n_events.clamp(min=0, max=self.max_events)

    @property
    def truncated(self):
        """[B] bool: the read has more events than the rows hold"""
        return self.n_events > self.max_events

    @property
    def length(self):
        """[B, max_events] int32: the samples of every event, 0 past the last one"""
        e = torch.arange(self.max_events, device=self.starts.device)[None, :]
        return torch.where(e < self.held[:, None], self.starts[:, 1:] - self.starts[:, :-1], torch.zeros_like(self.kind))

    @property
    def mean(self):
        """[B, max_events] float64: the level of every event in the units of v, NaN past the last one (one division of exact
        integers)"""
        return self.sum.double() / (self.length.double() * float(1 << self.frac_bits))

    @property
    def stdv(self):
        """[B, max_events] float64: the population standard deviation of every event, NaN past the last one; formed as
        KmerEvents.stdv"""
        n = self.length.double()
        m = self.sum.double() / n
        var = (self.sumsq.double() / n - m * m).clamp_(min=0.0)
        return var.sqrt() / float(1 << self.frac_bits)

    def as_signal(self):
        """(means [B, max_events] float32, lengths [B] int32): the event means as a shorter "read" -- 0 past the last event, and
        `held` events per read -- for signal_map and signal_align in place of the samples"""
        return torch.nan_to_num(self.mean, nan=0.0).float(), self.held.int()


def detect_events(signal, signal_lengths, scale_shift=None, frac_bits=12, windows=(3, 6), thresholds=DEFAULT_THRESHOLDS, radii=None,
                  min_var=DEFAULT_MIN_VAR, max_event_len=65536, max_events=None, chunk=None):
    """Event detection: where the level of a raw read changes, from the samples alone -- no bases, no
    network, no model -- and the table of the events between the changes.

    signal          [B, L] or [B, 1, L], float32 or int16; a view is passed by its row stride (unit stride along L)
    signal_lengths  [B]; scale_shift [B, 2] float32 or None, frac_bits: as kmer_events (q = round(v 2^frac_bits), |q| < 2^23)
    windows         (w_short, w_long), 1..16; w_long = 0 switches the long detector off.  The score of a position is Welch's t^2
                    between the w samples before it and the w samples from it on
    thresholds      (t_short, t_long) on t, as scrappie's; a position passes iff its t^2 is at least round(t^2 256) / 256
    radii           (r_short, r_long), 1..64 (None: the windows): a peak is the arg-max of its +-r neighbourhood, ties to the
                    smaller index
    min_var         the floor on var_1 + var_2 of the two windows in the units of v^2: a noise-free step has a finite score
    max_event_len   1..65536: a longer event is split every max_event_len samples
    max_events      the events the rows hold per read (None: L, which is always enough); n_events is the true count regardless
    chunk           the positions one workgroup decides, a multiple of 256 in [256, 16384] (None: chosen from L and B).  A tuning
                    argument: no output depends on it
    The boundaries are position 0, every short peak and every long peak with no short peak within +-w_long.  Integer arithmetic,
    exact 128-bit comparisons, bitwise reproducible, no host synchronisation (capturable with fixed shapes).  A bad read (a
    length out of range, a non-finite or out-of-range sample before signal_lengths[b]) is reported through check_device_flags().
    HIP only.  Returns DetectedEvents; its as_signal() goes into signal_map / signal_align as a read of event means."""
    what = "detect_events"
    signal = _args.signal_rows(signal, what)
    dev = signal.device
    B, L = int(signal.shape[0]), int(signal.shape[1])
    with torch.cuda.device(dev):
        signal_lengths = _args.lengths(signal_lengths, B, dev, what, "signal_lengths", flatten=True)
        scale_shift = _args.scale_shift(scale_shift, B, dev, what)
    F = int(frac_bits)
    radii = windows if radii is None else radii
    try:
        (w0, w1), (r0, r1), (t0, t1) = (int(v) for v in windows), (int(v) for v in radii), (float(v) for v in thresholds)
    except (TypeError, ValueError):
        raise ValueError("wavenet_speech_amd.%s: windows, thresholds and radii must be pairs (short, long)" % what) from None
    if not 0 <= F <= MAX_FRAC_BITS or not 1 <= w0 <= MAX_DETECT_WINDOW or not 0 <= w1 <= MAX_DETECT_WINDOW:
        raise ValueError("wavenet_speech_amd.%s: frac_bits in [0, %d], windows[0] in [1, %d], windows[1] in [0, %d]"
                         % (what, MAX_FRAC_BITS, MAX_DETECT_WINDOW, MAX_DETECT_WINDOW))
    if w1 == 0:
        r1, t1 = 1, 1.0                                              # unused
    min_var = float(min_var)
    if not all(1 <= r <= MAX_DETECT_RADIUS for r in (r0, r1)) or not all(math.isfinite(t) and t > 0 for t in (t0, t1)) \
            or not (math.isfinite(min_var) and min_var >= 0):
        raise ValueError("wavenet_speech_amd.%s: radii in [1, %d], thresholds finite and positive, min_var finite and >= 0"
                         % (what, MAX_DETECT_RADIUS))
    theta = [max(1, round(t * t * 256)) for t in (t0, t1)]
    vmin = [max(1, round(min_var * 4 ** F * w * w)) for w in (w0, max(w1, 1))]
    if max(theta) >= 2 ** 31 or max(vmin) > MAX_DETECT_VMIN:
        raise ValueError("wavenet_speech_amd.%s: round(t^2 256) must stay below 2^31 and round(min_var 4^frac_bits w^2) within 2^55" % what)
    max_event_len = int(max_event_len)
    N = L if max_events is None else int(max_events)
    chunk = 0 if chunk is None else int(chunk)
    chunk_ok = chunk == 0 or (chunk % 256 == 0 and MIN_CHUNK <= chunk <= MAX_CHUNK)
    if not 1 <= max_event_len <= MAX_EVENT_LEN or not 1 <= N <= MAX_DETECT_EVENTS or not chunk_ok:
        raise ValueError("wavenet_speech_amd.%s: max_event_len in [1, %d], max_events in [1, 2^24], chunk None or a multiple of 256 in "
                         "[%d, %d]" % (what, MAX_EVENT_LEN, MIN_CHUNK, MAX_CHUNK))
    if L > MAX_DETECT_SIGNAL or B > 65535:
        raise ValueError("wavenet_speech_amd.%s: at most 2^24 samples per read and 65535 reads, got %d and %d" % (what, L, B))
    with torch.cuda.device(dev):
        lib = _lib.load()
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        n_events, starts, kind = torch.empty(B, **i32), torch.empty(B, N + 1, **i32), torch.empty(B, N, **i32)
        ev_sum, ev_sumsq = torch.empty(B, N, **i64), torch.empty(B, N, **i64)
        bad = torch.zeros(1, **i32)
        ws = _alloc_bytes(lib.wn_event_detect_workspace_bytes(B, L), "wn_event_detect_workspace_bytes", dev, status=-2)
        _lib.check(lib.wn_event_detect(_p(signal), int(signal.dtype == torch.int16), signal.stride(0), _p(signal_lengths), _p(scale_shift),
                                       B, L, F, w0, w1, r0, r1, theta[0], theta[1], vmin[0], vmin[1], max_event_len, N, chunk,
                                       _p(n_events), _p(starts), _p(ev_sum), _p(ev_sumsq), _p(kind), _p(ws), ws.numel(), _p(bad),
                                       _stream()), "wn_event_detect")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.detect_events: %d bad read(s): a length out of range or a non-finite or "
                       "out-of-range sample" % n)
    return DetectedEvents(n_events, starts, ev_sum, ev_sumsq, kind, frac_bits=F)


MAX_MOVE_COST = 1 << 30
DEFAULT_MOVES = (0.14, 0.62, 0.20, 0.04)

_EventAlignFields = namedtuple("EventAlignment", "starts score band_hits moves states")


class EventAlignment(_Nats, _EventAlignFields):
    """starts [B, N + 1] int32: starts[b, j] is the first SAMPLE of state (k-mer) j -- RaggedReads.starts' convention, so it goes
    into kmer_events(starts=...) as it is; a skipped state is empty (starts[b, j] == starts[b, j + 1]; kmer_events gives it the code
    -2 and does not call the read bad) and every entry past the read's last state is the read's last sample + 1; score [B] int64: the
    cost of the path, move costs included, LLONG_MAX where there is no alignment and LLONG_MIN for a bad read; band_hits [B] int32:
    the events whose state lies on the band's edge while the band could still have been wider there; moves [B, 4] int32: the events
    that arrived by a stay, a step, a skip of one and a skip of two k-mers (1 + their sum is the read's events); states
    [B, max_events] int32 with want_states, else None: the state of every event, -1 past the read's events.  No alignment: starts
    and states -1, band_hits and moves 0; a bad read: everything -1.  Device tensors.  k, first, frac_bits, cost_bits, band and
    move_costs (the four integers the call ran with) ride along as attributes."""

    def __new__(cls, *fields, k=5, first=0, frac_bits=12, cost_bits=8, band=512, move_costs=(0, 0, 0, 0)):
        self = super().__new__(cls, *fields)
        self.k, self.first, self.frac_bits, self.cost_bits, self.band = int(k), int(first), int(frac_bits), int(cost_bits), int(band)
        self.move_costs = tuple(int(c) for c in move_costs)
        return self


def move_costs(probs, cost_bits=8):
    """The four integer move costs of event_align from the probabilities of advancing by 0 (stay), 1 (step), 2 and 3 k-mers
    between consecutive events: round(-ln p * 2^cost_bits), ties to even, in the units of a SignalModel with the same cost_bits;
    p = 0 forbids the move (-1).  The four need not sum to one.  Refused: anything but four finite values in [0, 1], a forbidden
    step, a cost at or above 2^30."""
    what = "move_costs"
    try:
        pp = [float(p) for p in probs]
    except (TypeError, ValueError):
        raise ValueError("wavenet_speech_amd.%s: probs must be four numbers" % what) from None
    cb = int(cost_bits)
    if len(pp) != 4 or not all(math.isfinite(p) and 0.0 <= p <= 1.0 for p in pp) or not 0 <= cb <= 16:
        raise ValueError("wavenet_speech_amd.%s: four finite probabilities in [0, 1] and cost_bits in [0, 16]" % what)
    if pp[1] == 0.0:
        raise ValueError("wavenet_speech_amd.%s: the step (probs[1]) cannot be forbidden" % what)
    out = tuple(-1 if p == 0.0 else round(-math.log(p) * (1 << cb)) + 0 for p in pp)          # + 0: no negative zero
    if max(out) >= MAX_MOVE_COST:
        raise ValueError("wavenet_speech_amd.%s: a move cost at or above 2^30" % what)
    return out


def fit_moves(move_counts):
    """The frequencies of the four moves over the good reads of an alignment: move_counts is EventAlignment.moves ([B, 4]
    integers; reads with a negative row -- bad ones -- are left out, reads without an alignment add nothing).  Returns four floats
    that sum to one, for event_align(moves=...): align -> fit_moves -> align re-estimates the move probabilities as align ->
    kmer_events -> fit_kmer_model re-estimates the table.  Raises if no move was counted or no step was."""
    rows = _host_table(move_counts, "fit_moves", "move_counts", 4)
    total = [sum(r[m] for r in rows if min(r) >= 0) for m in range(4)]
    if sum(total) < 1 or total[1] < 1:
        raise ValueError("wavenet_speech_amd.fit_moves: no move, or no step, among the good reads")
    return tuple(t / sum(total) for t in total)


def event_align(events, labels, label_lengths, model, first=0, band=512, moves=DEFAULT_MOVES, max_cost=None, want_states=False,
                frac_bits=None):
    """Align DETECTED events to the k-mers of known bases under a SignalModel: the minimum-cost path in
    which an event stays in the k-mer of the event before it (the detector cut one k-mer in two), steps to the next, or skips one
    or two k-mers (the detector missed boundaries), inside a band of `band` k-mers around the diagonal.  What nanopolish
    `eventalign` does; signal_align, which never skips, has no alignment for a read with fewer events than k-mers.

    events          a DetectedEvents (detect_events' result), or the tuple (n_events [B], starts [B, M + 1], sum [B, M], sumsq
                    [B, M]) with frac_bits=.  Of a DetectedEvents its `held` is passed as the count: a read that detection called
                    bad has no events and gets no alignment; a truncated read aligns the events its rows hold
    labels          [B, n] bases in 1..4 (int32 or int64) with label_lengths [B]
    model           a SignalModel; its k is the call's and its frac_bits must be the events'
    first           read b has label_lengths[b] - (k - 1) - 2 first states, as signal_align
    band            a multiple of 64 in [64, 2048]; state j is allowed at event e iff lo(e) <= j < lo(e) + band, lo(e) =
                    clamp(((2 e + 1) N) // (2 E) - band / 2, 0, max(N - band, 0))
    moves           four probabilities (floats), turned into costs by move_costs(moves, model.cost_bits), or four ints taken as
                    costs as they are (-1 forbids a move).  DEFAULT_MOVES = (0.14, 0.62, 0.20, 0.04): the stay and the total skip
                    mass are read off one sweep of the detector at noise 1.5 (14 % of the detected boundaries spurious, 28 % of
                    the true ones missed -- the latter a rate per true boundary used as a rate per event, an approximation) and
                    the split of the skips between one and two k-mers is a guess.  Nothing derives these numbers: fit_moves on a
                    first alignment gives the data's own
    max_cost        the clamp of a SAMPLE's quadratic term, in [1, 2^31 - 1] (None: 2^31 - 1); an event of n samples is clamped
                    at n max_cost
    want_states     also return the state of every event
    An event of n samples with sum S and sum of squares Q costs min((Q - 2 level S + n level^2) weight >> weight_shift,
    n max_cost) + n offset in a state: the exact sum of what signal_align charges its samples, up to one floor instead of n.
    Integer arithmetic, ties to the smallest move, bitwise reproducible, no host synchronisation (capturable with fixed shapes
    once the model has been used on the device).  A bad read (a length out of range, a label of the used window outside 1..4, a
    model row out of range, an event table that no samples could have made) is reported through check_device_flags().  HIP only.
    Returns EventAlignment."""
    what = "event_align"
    if isinstance(events, DetectedEvents):
        if frac_bits is not None and int(frac_bits) != events.frac_bits:
            raise ValueError("wavenet_speech_amd.%s: frac_bits=%d, but the events were made with %d" % (what, int(frac_bits), events.frac_bits))
        count, ev_starts, ev_sum, ev_sumsq, F = events.held, events.starts, events.sum, events.sumsq, events.frac_bits
    else:
        if not isinstance(events, (tuple, list)) or len(events) != 4 or frac_bits is None:
            raise ValueError("wavenet_speech_amd.%s: events must be a DetectedEvents, or (n_events, starts, sum, sumsq) with frac_bits=" % what)
        count, ev_starts, ev_sum, ev_sumsq = events
        F = int(frac_bits)
    call = _BandCall(what, model, first, band, max_cost, events_frac_bits=F)
    k, first, band, max_cost = call.k, call.first, call.band, call.max_cost
    try:
        moves = tuple(moves)
    except TypeError:
        raise ValueError("wavenet_speech_amd.%s: moves must be four probabilities or four integer costs" % what) from None
    if len(moves) == 4 and all(isinstance(m, int) and not isinstance(m, bool) for m in moves):
        costs = moves
        if costs[1] < 0 or not all(c == -1 or 0 <= c < MAX_MOVE_COST for c in costs):
            raise ValueError("wavenet_speech_amd.%s: a move cost is -1 (forbidden) or in [0, 2^30), and the step's is not -1" % what)
    else:
        costs = move_costs(moves, model.cost_bits)
    ev_starts = _args.gpu_tensor(ev_starts, what, "events.starts", (torch.int32,), ValueError)
    dev = ev_starts.device
    if ev_starts.dim() != 2 or ev_starts.shape[1] < 2:
        raise ValueError("wavenet_speech_amd.%s: events.starts must be [B, max_events + 1 >= 2], got %s" % (what, tuple(ev_starts.shape)))
    B, M = int(ev_starts.shape[0]), int(ev_starts.shape[1]) - 1
    ev_starts = ev_starts.contiguous()
    sums = []
    for name, t in (("sum", ev_sum), ("sumsq", ev_sumsq)):
        t = _args.gpu_tensor(t, what, "events." + name, (torch.int64,), ValueError, dev)
        if tuple(t.shape) != (B, M):
            raise ValueError("wavenet_speech_amd.%s: events.%s must be [%d, %d], got %s" % (what, name, B, M, tuple(t.shape)))
        sums.append(t.contiguous())
    labels = _args.int_rows(labels, what, "labels", B=B, shape="(%d, n >= 1)" % B, min_width=1, device=dev)
    with torch.cuda.device(dev):
        count = _args.lengths(count, B, dev, what, "n_events", flatten=True)
        label_lengths = _args.lengths(label_lengths, B, dev, what, "label_lengths", flatten=True)
    N = call.states(labels)
    if M > MAX_ALIGN_EVENTS or N > MAX_ALIGN_EVENTS or B > 65535:
        raise ValueError("wavenet_speech_amd.%s: at most 2^20 events and 2^20 k-mers per read and 65535 reads" % what)
    with torch.cuda.device(dev):
        lib = _lib.load()
        table = model.on(dev)
        starts, score, band_hits, bad = call.outputs(B, N, dev)
        counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
        states = torch.empty(B, M, dtype=torch.int32, device=dev) if want_states else None
        ws = _alloc_bytes(lib.wn_event_align_workspace_bytes(B, M, band), "wn_event_align_workspace_bytes", dev, status=-2)
        _lib.check(lib.wn_event_align(_p(count), _p(ev_starts), _p(sums[0]), _p(sums[1]), _p(labels), labels.stride(0), _p(label_lengths),
                                      _p(table), B, M, int(labels.shape[1]), N, k, first, F, model.weight_shift, max_cost, band, costs[0],
                                      costs[1], costs[2], costs[3], _p(starts), _p(score), _p(states), _p(counts), _p(band_hits), _p(ws),
                                      ws.numel(), _p(bad), _stream()), "wn_event_align")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.event_align: %d bad read(s): a length out of range, a label outside 1..4, a model "
                       "row out of range or an event whose length, sum and sum of squares no samples could have made" % n)
    return EventAlignment(starts, score, band_hits, counts, states, k=k, first=first, frac_bits=F, cost_bits=model.cost_bits, band=band,
                          move_costs=costs)
