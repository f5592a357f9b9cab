"""
Barcode demultiplexing and adapter trimming of decoded reads on the device (csrc/wn_demux.hip through
wn_demux_scores and wn_demux_pick): which sample a read of a multiplexed run belongs to, and where its adapters and barcodes end,
before the FASTQ is written -- what guppy, dorado, porechop and qcat do right after basecalling.

    labels, lengths, frames = ctc_greedy_decode(logits)
    kit = BarcodeSet(["AAGAAAGTTGTCGGTGTCTTTGTG", ...], front_flank="GGTGCTG", rear_flank="TTAACCT")
    d = demultiplex(labels, lengths, kit)                  # d.barcode [B], d.trim [B, 2], d.hits, d.runner_up, d.scores
    seq, n, q = trim_reads(labels, lengths, d.trim, qual=qualities.qual)
    print("".join(fastq_records(names, seq, n, q)))        # d.names(): the sample of every read

Every pattern is aligned SEMI-GLOBALLY with affine gaps against a window at the read's front or rear: the pattern is consumed whole,
its start and end in the window are free.  Scores are exact integers in half units, as in pairwise_align; among equally scoring
alignments the smallest start, then the smallest end is reported, which no order of evaluation can change.  Everything stays on the
device; nothing is copied to the host.  There is no CPU fallback: CPU tensors raise.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import _args, _lib
from ._args import _p, _stream
from .decoding import DEFAULT_ALPHABET

MAX_WINDOW = 512
MAX_PATTERNS = 1024
MAX_PATTERN_LEN = 128
MAX_READ_LEN = 1 << 24
DEFAULT_COMPLEMENT = (0, 4, 3, 2, 1)          # of " AGCT": A <-> T, G <-> C, the blank stays
# porechop's scoring scheme (match 3, mismatch -6, gap open -5, gap extend -2): a CHOICE in the spirit of porechop and guppy, not a
# value calibrated on this basecaller's errors; so are window=150 (porechop's end_size), min_fraction and min_margin below
DEFAULT_COSTS = dict(match=3, mismatch=-6, gap_open=5, gap_extend=2)
NO_RUNNER_UP = -2 ** 31


def _sequence(seq, what, name, alphabet):
    """one pattern as a list of labels: a string over `alphabet` or integers"""
    if isinstance(seq, str):
        try:
            return [alphabet.index(ch) for ch in seq]
        except ValueError:
            raise ValueError("wavenet_speech_amd.%s: %s %r has a character outside the alphabet %r" % (what, name, seq, alphabet))
    out = [int(v) for v in (seq.tolist() if hasattr(seq, "tolist") else seq)]
    return out


def _revcomp(seq, complement, what):
    if any(not 0 <= v < len(complement) for v in seq):
        raise ValueError("wavenet_speech_amd.%s: a label outside [0, %d) has no complement" % (what, len(complement)))
    return [int(complement[v]) for v in reversed(seq)]


def reverse_complement(labels, lengths, complement=DEFAULT_COMPLEMENT):
    """The reverse complement of every label row [B, L] over its own length [B], zero past it: torch ops on the device of `labels`
    (any device), no host sync.  complement[v] is the partner of label v; the default is that of DEFAULT_ALPHABET = " AGCT".  A
    label outside the table is clamped into it."""
    labels = torch.as_tensor(labels)
    if labels.dim() != 2 or labels.is_floating_point():
        raise ValueError("wavenet_speech_amd.reverse_complement: labels must be integers of shape (B, L), got %s %s"
                         % (labels.dtype, tuple(labels.shape)))
    B, L = labels.shape
    n = torch.as_tensor(lengths).to(device=labels.device, dtype=torch.int64).reshape(-1)
    if n.shape[0] != B:
        raise ValueError("wavenet_speech_amd.reverse_complement: lengths must hold %d lengths, got %d" % (B, n.shape[0]))
    if L == 0:
        return labels.clone()
    n = n.clamp(0, L)
    col = torch.arange(L, device=labels.device)
    src = (n[:, None] - 1 - col[None, :]).clamp(min=0)
    table = torch.as_tensor(list(complement), dtype=labels.dtype, device=labels.device)
    out = table[labels.gather(1, src).long().clamp(0, len(table) - 1)]
    return torch.where(col[None, :] < n[:, None], out, torch.zeros_like(out))


class BarcodeSet(object):
    """The pattern table of a barcode kit.  barcodes: strings over `alphabet`, or integer sequences, or a 2-d integer array with
    `lengths`.  Barcode g, written front_flank + barcode + rear_flank, is a FRONT pattern of group g; with both_ends=True its
    reverse complement is a REAR pattern of the same group.  extra_front / extra_rear: adapters (as they read at that end), each
    a group of its own after the barcodes -- a set of adapters alone gives pure trimming.  names: one per barcode (default
    "barcode01" ...); the adapters are named "front_adapter01" ... / "rear_adapter01" ...
    Patterns are sorted by end: [0, n_front) front, [n_front, K) rear.  Host arrays: patterns [K, Pmax] int32 zero-padded,
    pattern_lengths, pattern_end, pattern_group [K] int32; group_names.  K <= 1024, 1 <= every length <= 128."""

    def __init__(self, barcodes=(), lengths=None, names=None, front_flank=None, rear_flank=None, both_ends=True, extra_front=(),
                 extra_rear=(), alphabet=DEFAULT_ALPHABET, complement=DEFAULT_COMPLEMENT):
        what = "BarcodeSet"
        if lengths is not None:
            rows = np.asarray(barcodes.cpu() if isinstance(barcodes, torch.Tensor) else barcodes)
            ns = [int(v) for v in np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths).reshape(-1)]
            if rows.ndim != 2 or len(ns) != rows.shape[0] or any(not 0 <= n <= rows.shape[1] for n in ns):
                raise ValueError("wavenet_speech_amd.%s: with lengths, barcodes must be (n, L) rows and lengths n values in [0, L]" % what)
            barcodes = [rows[i, :n].tolist() for i, n in enumerate(ns)]
        codes = [_sequence(s, what, "barcode", alphabet) for s in barcodes]
        ff = _sequence(front_flank, what, "front_flank", alphabet) if front_flank is not None else []
        rf = _sequence(rear_flank, what, "rear_flank", alphabet) if rear_flank is not None else []
        if names is None:
            names = ["barcode%02d" % (i + 1) for i in range(len(codes))]
        names = [str(n) for n in names]
        if len(names) != len(codes):
            raise ValueError("wavenet_speech_amd.%s: %d names for %d barcodes" % (what, len(names), len(codes)))
        front = [(ff + c + rf, g) for g, c in enumerate(codes)]
        rear = [(_revcomp(p, complement, what), g) for p, g in front] if both_ends else []
        for end, extra, table in (("front", extra_front, front), ("rear", extra_rear, rear)):
            for i, s in enumerate(extra):
                table.append((_sequence(s, what, "adapter", alphabet), len(names)))
                names.append("%s_adapter%02d" % (end, i + 1))
        self._set(front, rear, names)

    @classmethod
    def from_table(cls, patterns, pattern_lengths, pattern_end, pattern_group, names=None):
        """a set from a finished table, for kits that the constructor cannot express (a barcode whose front and rear sequences
        differ: two patterns of one group): patterns [K, >= max length] integers with pattern_lengths, pattern_end (0 front, 1 rear)
        and pattern_group (>= 0) [K].  Front patterns are moved before rear ones, otherwise the order is kept."""
        rows = np.asarray(patterns)
        ns, ends, groups = ([int(v) for v in np.asarray(a).reshape(-1)] for a in (pattern_lengths, pattern_end, pattern_group))
        if rows.ndim != 2 or not (rows.shape[0] == len(ns) == len(ends) == len(groups)) or any(not 0 <= n <= rows.shape[1] for n in ns) \
                or any(e not in (0, 1) for e in ends) or any(g < 0 for g in groups):
            raise ValueError("wavenet_speech_amd.BarcodeSet: from_table needs (K, L) rows, K lengths in [0, L], K ends in {0, 1} and K groups >= 0")
        if names is None:
            names = ["group%02d" % g for g in range(max(groups) + 1)] if groups else []
        self = cls.__new__(cls)
        table = [(rows[k, :ns[k]].tolist(), groups[k], ends[k]) for k in range(len(ns))]
        self._set([(p, g) for p, g, e in table if e == 0], [(p, g) for p, g, e in table if e == 1], [str(n) for n in names])
        return self

    def _set(self, front, rear, names):
        what = "BarcodeSet"
        table = front + rear
        if not 1 <= len(table) <= MAX_PATTERNS:
            raise ValueError("wavenet_speech_amd.%s: need 1 to %d patterns, got %d" % (what, MAX_PATTERNS, len(table)))
        if any(not 1 <= len(p) <= MAX_PATTERN_LEN for p, _ in table):
            raise ValueError("wavenet_speech_amd.%s: every pattern (flanks included) must have 1 to %d labels, got %s"
                             % (what, MAX_PATTERN_LEN, sorted(set(len(p) for p, _ in table))))
        self.n_front, self.n_patterns = len(front), len(table)
        self.max_pattern_len = max(len(p) for p, _ in table)
        self.patterns = np.zeros((len(table), self.max_pattern_len), dtype=np.int32)
        for k, (p, _) in enumerate(table):
            self.patterns[k, :len(p)] = p
        self.pattern_lengths = np.array([len(p) for p, _ in table], dtype=np.int32)
        self.pattern_end = np.array([0] * len(front) + [1] * len(rear), dtype=np.int32)
        self.pattern_group = np.array([g for _, g in table], dtype=np.int32)
        self.group_names = names
        self._on = {}

    def on(self, device):
        """(patterns, pattern_lengths, pattern_group) on a device (uploaded once per device, so that a later call can be captured
        into a graph)"""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = tuple(torch.from_numpy(a).to(device) for a in (self.patterns, self.pattern_lengths, self.pattern_group))
        return self._on[device]

    def min_scores(self, min_fraction, match):
        """[K] integers in half units: ceil(min_fraction * 2 match * P_k), formed exactly"""
        frac = Fraction(min_fraction).limit_denominator(1000000)
        return [int(math.ceil(frac * int(2 * match) * int(P))) for P in self.pattern_lengths]


class DemuxScores(namedtuple("DemuxScores", "score start end")):
    """score [B, K] fp32 (the integer score x 0.5, as PairwiseAlignment.score; -2^30 for a poisoned entry); start, end [B, K] int32 in
    read coordinates, end exclusive, start == end where the pattern met only gaps, -1 for a poisoned entry.  Column k is pattern k
    of the BarcodeSet.  All on the device."""
    __slots__ = ()


class Demultiplexed(namedtuple("Demultiplexed", "barcode trim hits runner_up scores")):
    """barcode [B] int32: the group a read is assigned to, -1 for none; trim [B, 2] int32: the bases [trim_start, trim_end) that
    remain; hits [B, 2, 4] int32: per end (front, rear) the best pattern, its score IN HALF UNITS (the exact integer), start and
    end, four times -1 for an end without patterns; runner_up [B, 2] int32: the best score (half units) among that end's patterns
    of another group, -2^31 if there is none; scores: the DemuxScores they were picked from.  All on the device."""

    def names(self):
        """host helper: the name of every read's group, "unclassified" for -1 (one copy to the host)"""
        table = getattr(self, "group_names", None)
        return ["unclassified" if g < 0 else (table[g] if table is not None and g < len(table) else str(g))
                for g in self.barcode.cpu().tolist()]


def _scores(what, labels, lengths, patterns, window, costs):
    """the integer tables of wn_demux_scores with the checked rows and lengths they were made from"""
    if not isinstance(patterns, BarcodeSet):
        raise ValueError("wavenet_speech_amd.%s: patterns must be a BarcodeSet" % what)
    if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= MAX_WINDOW:
        raise ValueError("wavenet_speech_amd.%s: window must be an integer in [1, %d], got %r" % (what, MAX_WINDOW, window))
    labels = _args.int_rows(labels, what, "labels", pad_empty=True, lone_column_in_place=False)
    B, L = int(labels.shape[0]), int(labels.shape[1])
    dev = labels.device
    lengths = _args.lengths(lengths, B, dev, what, "lengths")
    if B < 1 or B > 65535 or L > MAX_READ_LEN:
        raise ValueError("wavenet_speech_amd.%s: need 1 to 65535 reads of at most %d labels, got %d of %d" % (what, MAX_READ_LEN, B, L))
    lib = _lib.load()
    K = patterns.n_patterns
    with torch.cuda.device(dev):
        pat, pat_len, _ = patterns.on(dev)
        score, start, end = (torch.empty(B, K, dtype=torch.int32, device=dev) for _ in range(3))
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_demux_scores(_p(labels), labels.stride(0), _p(lengths), _p(pat), pat.stride(0), _p(pat_len), B, L, K,
                                       patterns.n_front, patterns.max_pattern_len, int(window), costs[0], costs[1], costs[2], costs[3],
                                       _p(score), _p(start), _p(end), _p(bad), _stream()), "wn_demux_scores")
        _args.note_bad(bad, lambda n, L=L: "wavenet_speech_amd.%s: %d (read, pattern) entries of reads with a length outside [0, %d]"
                       % (what, n, L))
    return score, start, end, lengths


def demux_scores(labels, lengths, patterns, window=150, match=DEFAULT_COSTS["match"], mismatch=DEFAULT_COSTS["mismatch"],
                 gap_open=DEFAULT_COSTS["gap_open"], gap_extend=DEFAULT_COSTS["gap_extend"]):
    """Every pattern of a BarcodeSet against the front or rear window of every read.  labels [B, L] int32 or
    int64 GPU rows with lengths [B] -- what ctc_greedy_decode returned, or one beam of ctc_beam_decode, read in place through their
    row stride.  The window of a read of length n is labels[0 : min(n, window)] for a front pattern and labels[max(0, n - window) : n]
    for a rear one; window <= 512.  Costs must be multiples of 0.5 (the arithmetic is integer, in half units: exact); a gap of n
    columns costs gap_open + (n - 1) gap_extend.  The defaults are porechop's scoring scheme and end size: a choice, not a value
    calibrated for this basecaller.  Returns DemuxScores.  A read whose length is outside [0, L] poisons its row and is reported
    through check_device_flags()."""
    what = "demux_scores"
    costs = _args.affine_costs(what, match, mismatch, gap_open, gap_extend)
    score, start, end, _ = _scores(what, labels, lengths, patterns, window, costs)
    return DemuxScores(score.float() * 0.5, start, end)


def demultiplex(labels, lengths, patterns, window=150, match=DEFAULT_COSTS["match"], mismatch=DEFAULT_COSTS["mismatch"],
                gap_open=DEFAULT_COSTS["gap_open"], gap_extend=DEFAULT_COSTS["gap_extend"], min_fraction=0.6, min_margin=6.0,
                require_both=False):
    """demux_scores, then one decision per read, all on the device.  Per end the HIT is the pattern with the greatest score (ties to
    the lower index) and the runner-up the greatest score among that end's patterns of ANOTHER group.  A hit passes if its score is
    at least min_fraction of a perfect match of its pattern -- ceil(min_fraction * 2 match * P_k) in half units -- and leads the
    runner-up by at least min_margin (a multiple of 0.5 in score units; with no runner-up the margin holds).  barcode: with
    require_both the group of the front hit if both ends pass and agree, else -1; otherwise the group of the passing end with the
    greater score, a tie to the front.  trim: [end of the front hit if it passes, else 0; start of the rear hit (not before
    trim_start) if it passes, else the length).  min_fraction=0.6 and min_margin=6 (two matches) are a choice in the spirit of
    porechop's identity thresholds, not calibrated values.  Returns Demultiplexed."""
    what = "demultiplex"
    costs = _args.affine_costs(what, match, mismatch, gap_open, gap_extend)
    if not isinstance(patterns, BarcodeSet):
        raise ValueError("wavenet_speech_amd.%s: patterns must be a BarcodeSet" % what)
    if not (isinstance(min_fraction, (int, float)) and 0.0 <= float(min_fraction) <= 1.0):
        raise ValueError("wavenet_speech_amd.%s: min_fraction must be in [0, 1], got %r" % (what, min_fraction))
    margin = 2.0 * float(min_margin)
    if margin != int(margin) or not 0 <= margin < 2 ** 31:
        raise ValueError("wavenet_speech_amd.%s: min_margin must be a non-negative multiple of 0.5, got %r" % (what, min_margin))
    floors = patterns.min_scores(min_fraction, costs[0] / 2.0)
    score, start, end, lengths = _scores(what, labels, lengths, patterns, window, costs)
    B, K = int(score.shape[0]), int(score.shape[1])
    dev = score.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        key = ("min_score", dev, tuple(floors))
        if key not in patterns._on:                                  # uploaded once, so that a later call can be captured
            patterns._on[key] = torch.tensor(floors, dtype=torch.int32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        barcode, trim, hits, runner = torch.empty(B, **i32), torch.empty(B, 2, **i32), torch.empty(B, 2, 4, **i32), torch.empty(B, 2, **i32)
        _lib.check(lib.wn_demux_pick(_p(score), _p(start), _p(end), _p(lengths), _p(patterns.on(dev)[2]), _p(patterns._on[key]), B, K,
                                     patterns.n_front, int(margin), int(bool(require_both)), _p(barcode), _p(trim), _p(hits), _p(runner),
                                     _stream()), "wn_demux_pick")
    out = Demultiplexed(barcode, trim, hits, runner, DemuxScores(score.float() * 0.5, start, end))
    out.group_names = list(patterns.group_names)
    return out


def trim_reads(labels, lengths, trim, qual=None):
    """Cut every read to labels[trim_start : trim_end]: returns (rows [B, L] shifted to column 0 and zero past the new length, new
    lengths [B] int32) and, with qual [B, >= L], its rows shifted the same way as a third value.  trim [B, 2] is clamped into
    [0, length].  Torch ops on the device of `labels`, no host sync; the result goes straight into fastq_records."""
    what = "trim_reads"
    labels = torch.as_tensor(labels)
    if labels.dim() != 2 or labels.is_floating_point():
        raise ValueError("wavenet_speech_amd.%s: labels must be integers of shape (B, L), got %s %s" % (what, labels.dtype, tuple(labels.shape)))
    B, L = labels.shape
    dev = labels.device
    n = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).reshape(-1)
    trim = torch.as_tensor(trim).to(device=dev, dtype=torch.int64)
    if n.shape[0] != B or tuple(trim.shape) != (B, 2):
        raise ValueError("wavenet_speech_amd.%s: need %d lengths and trim of shape (%d, 2), got %s and %s"
                         % (what, B, B, tuple(n.shape), tuple(trim.shape)))
    if qual is not None:
        qual = torch.as_tensor(qual)
        if qual.dim() != 2 or qual.shape[0] != B or qual.shape[1] < L or qual.device != dev:
            raise ValueError("wavenet_speech_amd.%s: qual must be (%d, >= %d) on the device of the labels, got %s" % (what, B, L, tuple(qual.shape)))
    n = n.clamp(0, L)
    t0 = torch.minimum(trim[:, 0].clamp(min=0), n)
    t1 = torch.maximum(torch.minimum(trim[:, 1], n), t0)
    new_len = (t1 - t0).to(torch.int32)
    if L == 0:
        return (labels.clone(), new_len) if qual is None else (labels.clone(), new_len, qual[:, :0].clone())
    col = torch.arange(L, device=dev)
    src = (col[None, :] + t0[:, None]).clamp(max=L - 1)
    keep = col[None, :] < (t1 - t0)[:, None]
    rows = labels.gather(1, src)
    rows = torch.where(keep, rows, torch.zeros_like(rows))
    if qual is None:
        return rows, new_len
    q = qual[:, :L].gather(1, src)
    return rows, new_len, torch.where(keep, q, torch.zeros_like(q))
