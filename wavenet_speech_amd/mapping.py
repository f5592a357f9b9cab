"""
Signal-to-reference mapping under the k-mer pore model (csrc/wn_sigmap.hip through the C ABI's
wn_signal_map_reference and wn_signal_map): where on a known reference -- a plasmid, an amplicon, lambda, a bacterial genome --
the first second or so of a read's raw samples lies, on which strand, at what cost, and how far ahead of the next best locus that
is.  The subsequence form (start free, end free) of signal_align's dynamic program, under the same SignalModel; what UNCALLED,
sigmap and DTWax do for selective sequencing.  With it the loop of sections 7j / 7k closes on reads whose bases nobody supplied:

    model = signal_model(*standin_kmer_table())
    ref = map_reference(lambda_bases, model)                                               # once per (reference, model)
    hit = signal_map(signal[:, :2000], signal_lengths.clamp(max=2000), ref)                # where, which strand, how sure
    labels, label_lengths = hit.labels()
    al = signal_align(signal[:, :2000], signal_lengths.clamp(max=2000), labels, label_lengths, model, first=0, band=2048)
    ev = kmer_events(signal[:, :2000], signal_lengths.clamp(max=2000), labels, label_lengths, starts=al.starts, k=al.k, first=0)

HIP only: there is no CPU fallback.
"""
from collections import namedtuple

import torch

from . import _args, _lib
from ._args import _alloc_bytes, _p, _stream
from .events import SignalModel

GRANULE = 64                            # WN_MAP_GRANULE: the end states of one block of the block table
MAX_MAP_SIGNAL = 4096
MAX_MAP_REFERENCE = 1 << 26
MAX_STRIP = 1 << 20


def join_strands(bases):
    """bases + [0] + reverse_complement(bases) of a 1-d integer tensor: 1..4 become 5 - base, 0 (a break) and anything else stay as
    they are.  The 0 at the joint is a wall: no path crosses from one strand to the other."""
    bases = torch.as_tensor(bases)
    inside = (bases >= 1) & (bases <= 4)
    rc = torch.where(inside, 5 - bases, bases).flip(0)
    return torch.cat([bases, torch.zeros(1, dtype=bases.dtype, device=bases.device), rc])


class MapReference:
    """A reference prepared for signal_map: `bases` the int32 device tensor that is mapped against (both strands joined by a 0
    when both_strands), `prepared` the opaque device buffer of wn_signal_map_reference, `model` the SignalModel it was prepared
    under; R the bases of the forward strand, ref_len those of `bases`, k, and n_states = ref_len - k + 1."""

    def __init__(self, bases, prepared, model, R, both_strands):
        self.bases, self.prepared, self.model = bases, prepared, model
        self.R, self.ref_len, self.k, self.both_strands = int(R), int(bases.shape[0]), model.k, bool(both_strands)
        self.n_states = self.ref_len - self.k + 1
        self.device = bases.device


def map_reference(bases, model, both_strands=True, device=None):
    """Prepare a reference for signal_map (one launch, once per reference and model).

    bases         1-d integers: 1..4 for A C G T, 0 for a break (an N, a contig boundary); a list, or a tensor on any device
    model         a SignalModel; its k is the k-mer length
    both_strands  map against bases + [0] + reverse_complement(bases)
    device        where the reference lives (None: the device of `bases` if it is a GPU tensor, else the current GPU)
    A state (k-mer) whose window holds a 0 is a wall: no path is ever in it.  A base outside 0..4, or a k-mer whose model row is
    out of range, is treated the same and reported through check_device_flags().  Returns MapReference."""
    what = "map_reference"
    if not isinstance(model, SignalModel):
        raise ValueError("wavenet_speech_amd.%s: model must be a SignalModel (signal_model(means, stdvs)), got %s" % (what, type(model).__name__))
    bases = torch.as_tensor(bases)
    if bases.is_floating_point() or bases.dtype == torch.bool or bases.dim() != 1 or bases.shape[0] < 1:
        raise ValueError("wavenet_speech_amd.%s: bases must be 1-d integers (0..4) with at least one base, got %s %s"
                         % (what, bases.dtype, tuple(bases.shape)))
    R = int(bases.shape[0])
    ref_len = 2 * R + 1 if both_strands else R
    if R < model.k or ref_len > MAX_MAP_REFERENCE:
        raise ValueError("wavenet_speech_amd.%s: at least k = %d bases and at most 2^26 (both strands and the joint counted), got %d"
                         % (what, model.k, ref_len))
    if device is None:
        device = bases.device if bases.is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("wavenet_speech_amd.%s: the reference must live on a GPU (there is no CPU fallback)" % what)
    with torch.cuda.device(device):
        lib = _lib.load()
        bases = bases.detach().to(device=device, dtype=torch.int32)
        joined = (join_strands(bases) if both_strands else bases).contiguous()
        table = model.on(joined.device)
        prepared = _alloc_bytes(lib.wn_signal_map_reference_bytes(ref_len, model.k), "wn_signal_map_reference_bytes", joined.device, status=-2)
        bad = torch.zeros(1, dtype=torch.int32, device=joined.device)
        _lib.check(lib.wn_signal_map_reference(_p(joined), ref_len, _p(table), model.k, _p(prepared), prepared.numel(), _p(bad), _stream()),
                   "wn_signal_map_reference")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.map_reference: %d fault(s) in the reference: a base outside 0..4 or a k-mer "
                       "whose model row is out of range (treated as breaks)" % n)
    return MapReference(joined, prepared, model, R, both_strands)


_MapFields = namedtuple("SignalMapping", "score end start runner_up block_cost block_end end_cost")


class SignalMapping(_MapFields):
    """score [B] int64: the cost of the best path of the read's samples through the reference's states, start and end free; end,
    start [B] int32: its last and first state (state j is the k-mer bases[j .. j + k) of reference.bases), 0 <= end - start <
    signal_lengths[b]; runner_up [B] int64: the cost of the best path that ends signal_lengths[b] states or more away from `end`,
    in whole blocks (it shares no state with the best one); block_cost [B, ceil(n_states / 64)] int64 and block_end (int32): the
    minimum of the last row over the end states [64 g, 64 g + 64) and its smallest argmin; end_cost [B, n_states] int64 with
    want_end_cost, else None: the whole last row.  No mapping (no samples, or no finite cell): LLONG_MAX and -1; a bad read:
    LLONG_MIN and -1.  Device tensors.  The reference rides along as an attribute."""

    def __new__(cls, *fields, reference=None):
        self = super().__new__(cls, *fields)
        self.reference = reference
        self.k, self.cost_bits = reference.k, reference.model.cost_bits
        return self

    @property
    def mapped(self):
        return self.end >= 0

    @property
    def nats(self):
        """[B] float64: score / 2^cost_bits (the sentinels stay huge: mask with `mapped` first)"""
        return self.score.double() / float(1 << self.cost_bits)

    @property
    def strand(self):
        """[B] int32: 0 forward, 1 reverse, -1 where unmapped"""
        ref = self.reference
        rev = (self.end > ref.R).int() if ref.both_strands else torch.zeros_like(self.end)
        return torch.where(self.mapped, rev, torch.full_like(self.end, -1))

    def ref_span(self):
        """[B, 2] int64: the half-open range of forward-strand bases the read covers, (-1, -1) where unmapped.  Forward strand:
        [start, end + k); reverse strand, with s' = start - (R + 1) and e' = end - (R + 1): [R - e' - k, R - s')."""
        R, k = self.reference.R, self.k
        s, e = self.start.long(), self.end.long()
        fwd = torch.stack([s, e + k], dim=1)
        rev = torch.stack([R - (e - (R + 1)) - k, R - (s - (R + 1))], dim=1)
        span = torch.where((self.strand == 1)[:, None], rev, fwd)
        return torch.where(self.mapped[:, None], span, torch.full_like(span, -1))

    def labels(self):
        """(labels [B, nmax] int32, label_lengths [B] int32): reference.bases[start .. end + k) of every read, in read orientation
        (the reverse strand is part of reference.bases), zero-padded; length 0 where unmapped.  They go into signal_align(...,
        first=0) as they stand: end - start + 1 states, never more than the read has samples."""
        k, bases = self.k, self.reference.bases
        mapped = self.mapped
        length = torch.where(mapped, self.end - self.start + k, torch.zeros_like(self.end))
        nmax = max(int(length.max()), 1)
        idx = self.start.clamp(min=0).long()[:, None] + torch.arange(nmax, device=bases.device)[None, :]
        inside = torch.arange(nmax, device=bases.device)[None, :] < length[:, None]
        rows = bases[idx.clamp(max=bases.shape[0] - 1)]
        return torch.where(inside, rows, torch.zeros_like(rows)).contiguous(), length.int()


def signal_map(signal, signal_lengths, reference, scale_shift=None, max_cost=None, strip=None, want_end_cost=False):
    """Map the first samples of every read against a prepared reference: the minimum-cost path of the
    samples through consecutive k-mers of the reference, starting and ending anywhere, every sample staying in its k-mer or
    stepping to the next one (no skips), never through a break.

    signal          [B, L] or [B, 1, L], float32 or int16, L <= 4096; a view is passed by its row stride (unit stride along L)
    signal_lengths  [B]: the samples of each read that are mapped (hand in the prefix you want mapped: about a second of signal).
                    The event means of detect_events(...).as_signal() are such a read too: 4096 events instead of 4096 samples
    reference       a MapReference (map_reference(bases, model)) on the signal's device
    scale_shift     [B, 2] float32 or None, as kmer_events and signal_align
    max_cost        the clamp of a sample's quadratic term, in [1, 2^31 - 1] (None: 2^31 - 1), as signal_align
    strip           the end states one workgroup owns, a multiple of 64 in [64, 2^20] (None: chosen from L, the reference and B).
                    A tuning argument: no output depends on it
    want_end_cost   also return the whole last row [B, n_states]
    Integer arithmetic, ties to the stay and to the smallest end, bitwise reproducible for any strip, no host synchronisation
    (capturable with fixed shapes).  A bad read (a length out of range, a non-finite or out-of-range sample before
    signal_lengths[b]) is reported through check_device_flags().  HIP only.  Returns SignalMapping."""
    what = "signal_map"
    signal = _args.signal_rows(signal, what)
    dev = signal.device
    B, L = int(signal.shape[0]), int(signal.shape[1])
    if not isinstance(reference, MapReference):
        raise ValueError("wavenet_speech_amd.%s: reference must be a MapReference (map_reference(bases, model)), got %s"
                         % (what, type(reference).__name__))
    if reference.device != dev:
        raise ValueError("wavenet_speech_amd.%s: reference must be on %s" % (what, dev))
    with torch.cuda.device(dev):
        signal_lengths = _args.lengths(signal_lengths, B, dev, what, "signal_lengths", flatten=True)
        scale_shift = _args.scale_shift(scale_shift, B, dev, what)
    max_cost = 2 ** 31 - 1 if max_cost is None else int(max_cost)
    strip = 0 if strip is None else int(strip)
    if not 1 <= max_cost <= 2 ** 31 - 1 or (strip != 0 and (strip % GRANULE != 0 or not GRANULE <= strip <= MAX_STRIP)):
        raise ValueError("wavenet_speech_amd.%s: max_cost in [1, 2^31 - 1], strip None or a multiple of 64 in [64, 2^20]" % what)
    if L > MAX_MAP_SIGNAL or B > 65535:
        raise ValueError("wavenet_speech_amd.%s: at most 4096 samples per read (map a prefix) and 65535 reads, got %d and %d" % (what, L, B))
    model, k, M = reference.model, reference.k, reference.n_states
    G = (M + GRANULE - 1) // GRANULE
    with torch.cuda.device(dev):
        lib = _lib.load()
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        score, runner_up, block_cost = torch.empty(B, **i64), torch.empty(B, **i64), torch.empty(B, G, **i64)
        end, start, block_end = torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(B, G, **i32)
        end_cost = torch.empty(B, M, **i64) if want_end_cost else None
        bad = torch.zeros(1, **i32)
        ws = _alloc_bytes(lib.wn_signal_map_workspace_bytes(B, L, reference.ref_len, k, strip), "wn_signal_map_workspace_bytes", dev, status=-2)
        _lib.check(lib.wn_signal_map(_p(signal), int(signal.dtype == torch.int16), signal.stride(0), _p(signal_lengths), _p(scale_shift),
                                     _p(reference.prepared), reference.ref_len, k, B, L, model.frac_bits, model.weight_shift, max_cost,
                                     strip, _p(score), _p(end), _p(start), _p(runner_up), _p(block_cost), _p(block_end), _p(end_cost),
                                     _p(ws), ws.numel(), _p(bad), _stream()), "wn_signal_map")
        _args.note_bad(bad, lambda n: "wavenet_speech_amd.signal_map: %d bad read(s): a length out of range or a non-finite or "
                       "out-of-range sample" % n)
    return SignalMapping(score, end, start, runner_up, block_cost, block_end, end_cost, reference=reference)
