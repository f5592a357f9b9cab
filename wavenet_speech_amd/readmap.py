"""
Read mapping in base space on the device (csrc/wn_readmap.hip through wn_minimizers, wn_read_seeds and
wn_chain): which stretch of a reference, on which strand, a decoded read came from -- the step minimap2 runs after basecalling.
For a real read nobody knows the true bases; what one has is a reference, and the mapped stretch of it is what pairwise_align,
quality_profile, Basecaller.calibrate and fit_quality_calibration take as the truth.

    index = read_index(reference_bases)                                # once per reference: sketch and sort
    labels, lengths, frames = ctc_greedy_decode(logits)
    m = map_reads(labels, lengths, index)                              # m.score, m.strand, m.ref_start, ... [B], on the device
    ref, ref_lengths = m.labels(flank=20)                              # the mapped stretch in read orientation
    aln = pairwise_align(ref, ref_lengths, labels, lengths)
    print("".join(paf_records(names, lengths, m, "chr", alignment=aln)))

The read is sketched into minimizers (k-mers whose hash is the least of some window of w), the minimizers are looked up in the
sorted index of the reference's, and colinear hits are chained by minimap2's dynamic program.  Everything the kernels write is an
integer and every rule is a lexicographic maximum over a set, so results do not depend on any order of evaluation and equal the
host reference of tests/readmap_ref.py exactly.  map_reads does not synchronise with the host (fixed shapes capture into a graph);
read_index may.  There is no CPU fallback: CPU tensors raise.

Labels are the decoders': 1..4 are bases whose complement is 5 - v (DEFAULT_ALPHABET " AGCT"); anything else, 0 included, is a break.
The defaults (k=15, w=10, max_occ=8, h=64, max_dist=5000, bandwidth=500, gap_base=2, gap_log=8, anchors_per_read=4096) follow
minimap2's map-ont preset in spirit: a CHOICE, not calibrated on this basecaller's errors.  gap_base and gap_log are in sixteenths
of a base (0.01 k and 0.5 per log2).  Scores are in sixteenths of a base too and stay at or below 16 * 16 * 32768 = 2^23.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _args, _lib
from ._args import _p, _stream

MAX_K = 16
MAX_W = 64
MAX_OCC = 64
MAX_H = 1024
MAX_ANCHORS = 32768
MAX_READ_LEN = 65535
MAX_REFERENCE = 1 << 26
MAX_DIST = 1 << 26
MAX_GAP = 1024
MAX_CHUNK = 2048
STRAND_SHIFT, REF_SHIFT = 43, 16              # anchor word: s << 43 | r << 16 | q'
INDEX_SHIFT = 28                              # index word: canon << 28 | pos << 1 | strand
PAD = 2 ** 63 - 1
UNMAPPED = -2 ** 31


def _int_in(what, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("wavenet_speech_amd.%s: %s must be an integer in [%d, %d], got %r" % (what, name, lo, hi, v))
    return int(v)


def _rows(what, labels, lengths, max_len):
    labels = _args.int_rows(labels, what, "labels", pad_empty=True, lone_column_in_place=False)
    B, L = int(labels.shape[0]), int(labels.shape[1])
    if B < 1 or B > 65535 or L > max_len:
        raise ValueError("wavenet_speech_amd.%s: need 1 to 65535 rows of at most %d labels, got %d of %d" % (what, max_len, B, L))
    return labels, _args.lengths(lengths, B, labels.device, what, "lengths"), B, L


class Minimizers(namedtuple("Minimizers", "code flag")):
    """code [B, L] int32: the canonical code of the k-mer at a minimizer (its 32 bits; 0 elsewhere); flag [B, L] uint8: 0 no
    minimizer, 1 the forward code is canonical, 2 the reverse complement's.  On the device."""
    __slots__ = ()

    def compact(self):
        """(positions [B, nmax] int32, -1 past the count; codes [B, nmax] int64 in [0, 2^32); strands [B, nmax] int32 0 / 1;
        counts [B] int32) by torch ops (one host sync for nmax)"""
        on = self.flag > 0
        counts = on.sum(1).int()
        nmax = max(int(counts.max()), 1)
        order = torch.sort((~on).to(torch.uint8), dim=1, stable=True).indices[:, :nmax]
        inside = torch.arange(nmax, device=on.device)[None, :] < counts[:, None]
        codes = self.code.gather(1, order).long() & 0xFFFFFFFF
        strands = self.flag.gather(1, order).int() - 1
        zero = torch.zeros_like(codes)
        return (torch.where(inside, order, torch.full_like(order, -1)).int(), torch.where(inside, codes, zero),
                torch.where(inside, strands, torch.zeros_like(strands)), counts)


def _sketch(what, labels, lengths, B, L, k, w, chunk, report=True):
    dev = labels.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        code = torch.empty(B, L, dtype=torch.int32, device=dev)
        flag = torch.empty(B, L, dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev) if report else None
        _lib.check(lib.wn_minimizers(_p(labels), labels.stride(0), _p(lengths), B, L, k, w, chunk, _p(code), _p(flag), _p(bad), _stream()),
                   "wn_minimizers")
        _args.note_bad(bad, lambda n, L=L: "wavenet_speech_amd.%s: %d row(s) with a length outside [0, %d] (sketched as empty)" % (what, n, L))
    return Minimizers(code, flag)


def _chunk_arg(what, chunk):
    """the C ABI's chunk: 0 leaves the choice to the library"""
    return 0 if chunk is None else _int_in(what, "chunk", chunk, 1, MAX_CHUNK)


def _sketch_args(what, k, w, chunk):
    return _int_in(what, "k", k, 1, MAX_K), _int_in(what, "w", w, 1, MAX_W), _chunk_arg(what, chunk)


def minimizers(labels, lengths, k=15, w=10, chunk=None):
    """The (w, k) minimizers of every label row.  labels [B, L] int32 or int64 GPU rows with lengths [B], read
    in place through their row stride; L <= 2^26, so a whole reference is one row.  1 <= k <= 16, 1 <= w <= 64.  A k-mer with a break
    in it, or one that equals its reverse complement, is never a minimizer.  chunk: positions per workgroup, [1, 2048] (None: the
    library's choice); a tuning argument that no output depends on.  Returns Minimizers, dense [B, L]; a length outside [0, L] is
    reported through check_device_flags()."""
    what = "minimizers"
    k, w, chunk = _sketch_args(what, k, w, chunk)
    labels, lengths, B, L = _rows(what, labels, lengths, MAX_REFERENCE)
    return _sketch(what, labels, lengths, B, L, k, w, chunk)


class ReadIndex(object):
    """The minimizer index of a reference: `entries` [max(n_entries, 1)] int64 on the device, ascending, one word canon << 28 |
    pos << 1 | strand per minimizer (sorted by (canon, pos)); `bases` the int32 device tensor it was made from, R its length, k, w."""

    def __init__(self, entries, n_entries, bases, k, w):
        self.entries, self.n_entries, self.bases = entries, int(n_entries), bases
        self.R, self.k, self.w, self.device = int(bases.shape[0]), int(k), int(w), bases.device


def read_index(bases, k=15, w=10, device=None):
    """Sketch a reference and sort its minimizers: once per reference (torch.nonzero and torch.sort synchronise here).
    bases: 1-d integers as for map_reference, 1..4 with 0 (or anything else) a break -- an N, a contig boundary: no k-mer spans
    one, so breaks separate contigs; a list or a tensor on any device, at most 2^26.  device: where the index lives (None: the
    device of `bases` if it is a GPU tensor, else the current GPU).  Returns ReadIndex."""
    what = "read_index"
    k, w, _ = _sketch_args(what, k, w, None)
    bases = torch.as_tensor(bases)
    if bases.is_floating_point() or bases.dtype == torch.bool or bases.dim() != 1 or not 1 <= bases.shape[0] <= MAX_REFERENCE:
        raise ValueError("wavenet_speech_amd.%s: bases must be 1-d integers, 1 to 2^26 of them, got %s %s" % (what, bases.dtype, tuple(bases.shape)))
    if device is None:
        device = bases.device if bases.is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("wavenet_speech_amd.%s: the index must live on a GPU (there is no CPU fallback)" % what)
    with torch.cuda.device(device):
        bases = bases.detach().to(device=device, dtype=torch.int32).contiguous()
        R = int(bases.shape[0])
        sketch = _sketch(what, bases[None, :], torch.full((1,), R, dtype=torch.int32, device=bases.device), 1, R, k, w, 0)
        pos = torch.nonzero(sketch.flag[0]).reshape(-1)
        canon = sketch.code[0][pos].long() & 0xFFFFFFFF
        entries = (canon << INDEX_SHIFT) | (pos << 1) | (sketch.flag[0][pos].long() - 1)
        entries = torch.sort(entries).values
        n = int(entries.shape[0])
        if n == 0:
            entries = torch.full((1,), PAD, dtype=torch.int64, device=bases.device)
    return ReadIndex(entries.contiguous(), n, bases, k, w)


class Anchors(object):
    """The anchors of B reads, ready for chain_anchors: keys [B, cap] int64, every row ascending, one word s << 43 | r << 16 | q' per
    anchor (strand, reference position, position in the read as it maps: reverse-complemented when s = 1), then INT64_MAX;
    n_anchors [B] int32 (kept), n_minimizers [B] int32, truncated [B] int32 (1: there were more than cap); lengths [B] int32 and
    max_len: the reads' lengths and row width; k.  `reference`: the ReadIndex they were seeded from, or None."""

    def __init__(self, keys, n_anchors, n_minimizers, truncated, lengths, k, max_len, reference=None):
        self.keys, self.n_anchors, self.n_minimizers, self.truncated = keys, n_anchors, n_minimizers, truncated
        self.lengths, self.k, self.max_len, self.reference = lengths, int(k), int(max_len), reference

    def _field(self, v):
        return torch.where(self.keys == PAD, torch.full_like(self.keys, -1), v).int()

    @property
    def strand(self):
        """[B, cap] int32: 0 forward, 1 reverse, -1 for a pad"""
        return self._field((self.keys >> STRAND_SHIFT) & 1)

    @property
    def ref_pos(self):
        return self._field((self.keys >> REF_SHIFT) & ((1 << 27) - 1))

    @property
    def query_pos(self):
        return self._field(self.keys & 0xFFFF)

    def to(self, device):
        t = [None if x is None else x.to(device) for x in (self.keys, self.n_anchors, self.n_minimizers, self.truncated, self.lengths)]
        return Anchors(t[0], t[1], t[2], t[3], t[4], self.k, self.max_len, self.reference)

    @classmethod
    def from_table(cls, rows, counts, lengths, k, max_len=None, device=None):
        """Anchors from hand-made rows, so that chaining can be run on crafted input: rows [B, cap, 3] integers (s, r, q') with
        counts [B] (the first counts[b] rows of read b are used, in any order), lengths [B] the reads' lengths, k.  s in {0, 1},
        0 <= r < 2^26, 0 <= q' < 65536, the anchors of a read pairwise distinct.  max_len: the reads' row width (None: the greatest
        length, at least 1).  Built on the host; device=None leaves it there (chain_anchors wants it on a GPU: .to(device))."""
        what = "Anchors.from_table"
        rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows)
        counts = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts).reshape(-1)
        lengths = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths).reshape(-1)
        k = _int_in(what, "k", k, 1, MAX_K)
        if rows.ndim != 3 or rows.shape[2] != 3 or rows.dtype.kind not in "iu" or not 1 <= rows.shape[0] <= 65535 or \
                not 1 <= rows.shape[1] <= MAX_ANCHORS or counts.shape != (rows.shape[0],) or lengths.shape != (rows.shape[0],):
            raise ValueError("wavenet_speech_amd.%s: rows must be integers of shape (B, cap, 3) with 1 <= B <= 65535 and 1 <= cap <= %d, "
                             "counts and lengths (B,)" % (what, MAX_ANCHORS))
        B, cap = rows.shape[0], rows.shape[1]
        if any(not 0 <= int(c) <= cap for c in counts):
            raise ValueError("wavenet_speech_amd.%s: counts must lie in [0, %d]" % (what, cap))
        max_len = max(1, int(lengths.max())) if max_len is None else _int_in(what, "max_len", max_len, 1, MAX_READ_LEN)
        keys = np.full((B, cap), PAD, dtype=np.int64)
        for b in range(B):
            part = rows[b, :int(counts[b])].astype(np.int64)
            if part.size and (part[:, 0].min() < 0 or part[:, 0].max() > 1 or part[:, 1].min() < 0 or part[:, 1].max() >= MAX_REFERENCE
                              or part[:, 2].min() < 0 or part[:, 2].max() > 0xFFFF):
                raise ValueError("wavenet_speech_amd.%s: need s in {0, 1}, 0 <= r < 2^26 and 0 <= q' < 65536 (read %d)" % (what, b))
            word = np.sort((part[:, 0] << STRAND_SHIFT) | (part[:, 1] << REF_SHIFT) | part[:, 2])
            if word.size > 1 and (word[1:] == word[:-1]).any():
                raise ValueError("wavenet_speech_amd.%s: the anchors of read %d are not pairwise distinct" % (what, b))
            keys[b, :word.size] = word
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        out = cls(torch.from_numpy(keys), i32(counts), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32), i32(lengths),
                  k, max_len)
        return out if device is None else out.to(device)


def _seed_args(what, index, max_occ, anchors_per_read):
    if not isinstance(index, ReadIndex):
        raise ValueError("wavenet_speech_amd.%s: index must be a ReadIndex (read_index(bases)), got %s" % (what, type(index).__name__))
    return _int_in(what, "max_occ", max_occ, 1, MAX_OCC), _int_in(what, "anchors_per_read", anchors_per_read, 1, MAX_ANCHORS)


def _seed(what, labels, lengths, index, max_occ, cap, chunk, report=True):
    """report=False: the caller's next step counts the same bad lengths (one report per call)"""
    labels, lengths, B, L = _rows(what, labels, lengths, MAX_READ_LEN)
    dev = labels.device
    if index.device != dev:
        raise ValueError("wavenet_speech_amd.%s: index must be on %s" % (what, dev))
    sketch = _sketch(what, labels, lengths, B, L, index.k, index.w, chunk, report)
    lib = _lib.load()
    with torch.cuda.device(dev):
        keys = torch.empty(B, cap, dtype=torch.int64, device=dev)
        n_min, n_anchors, truncated = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
        _lib.check(lib.wn_read_seeds(_p(sketch.code), _p(sketch.flag), _p(lengths), _p(index.entries), index.n_entries, B, L, index.k,
                                     max_occ, cap, _p(keys), _p(n_min), _p(n_anchors), _p(truncated), None, _stream()), "wn_read_seeds")
    return Anchors(keys, n_anchors, n_min, truncated, lengths, index.k, L, reference=index)


def seed_anchors(labels, lengths, index, max_occ=8, anchors_per_read=4096, chunk=None):
    """Sketch every read with the index's k and w, look its minimizers up in the index and write the sorted anchor rows.  labels
    [B, L] int32 or int64 GPU rows (L <= 65535) with lengths [B].  A minimizer whose k-mer has more than max_occ (<= 64) entries in
    the index is dropped with all of them; of the anchors in enumeration order (minimizers by position, entries by reference
    position) the first anchors_per_read (<= 32768) are kept and `truncated` says whether there were more.  Returns Anchors."""
    what = "seed_anchors"
    max_occ, cap = _seed_args(what, index, max_occ, anchors_per_read)
    chunk = _chunk_arg(what, chunk)
    return _seed(what, labels, lengths, index, max_occ, cap, chunk)


_MapFields = namedtuple("ReadMapping", "score strand ref_start ref_end query_start query_end n_anchors runner_up f pred")


class ReadMapping(_MapFields):
    """Per read, [B] int32 on the device: score (the best chain's, in sixteenths of a base; -2^31 where unmapped), strand (0 forward,
    1 reverse, -1), [ref_start, ref_end) on the reference's forward strand, [query_start, query_end) in read orientation (-1 where
    unmapped), n_anchors (of the best chain), runner_up (the greatest score of an anchor on another chain: another strand or
    another root; -2^31 if there is none).  f, pred [B, cap] int32 with want_pred, else None: the whole chain table over the sorted
    anchor rows, pred an index into the row, -1 for a fresh start (past n_anchors: -2^31 and -1).  `anchors` rides along, and with it
    the reference, the reads' lengths and k."""

    def __new__(cls, *fields, anchors=None):
        self = super().__new__(cls, *fields)
        self.anchors = anchors
        self.reference, self.k, self.lengths = anchors.reference, anchors.k, anchors.lengths
        return self

    @property
    def mapped(self):
        return self.strand >= 0

    def ref_span(self):
        """[B, 2] int64: [ref_start, ref_end) on the forward strand, (-1, -1) where unmapped"""
        return torch.stack([self.ref_start.long(), self.ref_end.long()], dim=1)

    def labels(self, flank=0):
        """(rows [B, nmax] int32, lengths [B] int32): the mapped stretch of the reference widened by `flank` bases on either side and
        clamped to the reference, in READ orientation (the reverse strand reverse-complemented), zero-padded; length 0 where
        unmapped.  It goes into pairwise_align(rows, lengths, query, query_lengths) as it stands.  One host sync (nmax)."""
        what = "ReadMapping.labels"
        if self.reference is None:
            raise ValueError("wavenet_speech_amd.%s: these anchors were not seeded from a ReadIndex" % what)
        flank = _int_in(what, "flank", flank, 0, MAX_REFERENCE)
        bases, R = self.reference.bases, self.reference.R
        mapped = self.mapped
        lo = (self.ref_start.long() - flank).clamp(min=0)
        hi = (self.ref_end.long() + flank).clamp(max=R)
        length = torch.where(mapped, hi - lo, torch.zeros_like(lo))
        nmax = max(int(length.max()), 1)
        col = torch.arange(nmax, device=bases.device)[None, :]
        rev = (self.strand == 1)[:, None]
        idx = torch.where(rev, hi[:, None] - 1 - col, lo[:, None] + col).clamp(0, R - 1)
        rows = bases[idx]
        rows = torch.where(rev & (rows >= 1) & (rows <= 4), 5 - rows, rows)
        return torch.where(col < length[:, None], rows, torch.zeros_like(rows)).contiguous(), length.int()

    def window(self, flank=0):
        """(lo [B] int32, length [B] int32) on the device: the forward-strand position of the first base of the window that
        labels(flank) cuts out, and the window's length (0 where unmapped).  Column c of the row labels(flank) returns is forward
        position lo + c on strand 0 and lo + length - 1 - c on strand 1: what pileup() takes beside the alignment of that row.  No
        host synchronisation."""
        what = "ReadMapping.window"
        if self.reference is None:
            raise ValueError("wavenet_speech_amd.%s: these anchors were not seeded from a ReadIndex" % what)
        flank = _int_in(what, "flank", flank, 0, MAX_REFERENCE)
        lo = (self.ref_start.long() - flank).clamp(min=0)
        hi = (self.ref_end.long() + flank).clamp(max=self.reference.R)
        return lo.int(), torch.where(self.mapped, hi - lo, torch.zeros_like(lo)).int()

    def band(self, flank=0, margin=64, max_band=None):
        """(diag_lo, diag_hi), [B] int32 on the device: the stripe of diagonals j - i that banded_align(rows, lengths, query,
        query_lengths, ...) takes for the rows labels(flank) returns against the whole reads -- the diagonals of the chain's two end
        points in those rows' coordinates, widened by `margin` on each side and, with max_band, clamped about the centre to that width
        (DESIGN.md 7ab).  With (lo, n) = window(flank) the end points are query_start - (ref_start - lo) and query_end - (ref_end - lo)
        on strand 0, query_start - (lo + n - ref_end) and query_end - (lo + n - ref_start) on strand 1.  (0, 0) where unmapped: the
        window's length is 0.  No host synchronisation."""
        from .decoding import _clamp_band
        what = "ReadMapping.band"
        margin = _int_in(what, "margin", margin, 0, MAX_REFERENCE)
        lo, n = self.window(flank)
        lo, n = lo.long(), n.long()
        rs, re, qs, qe = (t.long() for t in (self.ref_start, self.ref_end, self.query_start, self.query_end))
        rev = self.strand == 1
        d0 = qs - torch.where(rev, lo + n - re, rs - lo)
        d1 = qe - torch.where(rev, lo + n - rs, re - lo)
        zero = torch.zeros_like(d0)
        dlo = torch.where(self.mapped, torch.minimum(d0, d1) - margin, zero)
        dhi = torch.where(self.mapped, torch.maximum(d0, d1) + margin, zero)
        dlo, dhi = _clamp_band(dlo, dhi, max_band)
        return dlo.int(), dhi.int()

    def mapq(self):
        """[B] float32 on the device: minimap2's formula 40 (1 - runner_up / score) min(1, n_anchors / 10) ln(score / 16), clamped to
        [0, 60]; a missing runner-up counts as 0; 0 where unmapped.  A CHOICE taken over from minimap2, not calibrated here."""
        s = self.score.double().clamp(min=16.0)
        ru = torch.where(self.runner_up == UNMAPPED, torch.zeros_like(s), self.runner_up.double())
        q = 40.0 * (1.0 - ru / s) * (self.n_anchors.double() / 10.0).clamp(max=1.0) * torch.log(s / 16.0)
        return torch.where(self.mapped, q.clamp(0.0, 60.0), torch.zeros_like(q)).float()


def _chain_args(what, h, max_dist, bandwidth, gap_base, gap_log):
    return (_int_in(what, "h", h, 1, MAX_H), _int_in(what, "max_dist", max_dist, 1, MAX_DIST), _int_in(what, "bandwidth", bandwidth, 1, MAX_DIST),
            _int_in(what, "gap_base", gap_base, 0, MAX_GAP), _int_in(what, "gap_log", gap_log, 0, MAX_GAP))


def _chain(what, anchors, args, want_pred):
    if not isinstance(anchors, Anchors):
        raise ValueError("wavenet_speech_amd.%s: anchors must be Anchors (seed_anchors(...) or Anchors.from_table(...)), got %s"
                         % (what, type(anchors).__name__))
    keys = _args.gpu_tensor(anchors.keys, what, "anchors.keys", (torch.int64,))
    dev = keys.device
    if keys.dim() != 2 or not 1 <= keys.shape[0] <= 65535 or not 1 <= keys.shape[1] <= MAX_ANCHORS:
        raise ValueError("wavenet_speech_amd.%s: anchors.keys must be (B, cap) with 1 <= B <= 65535 and 1 <= cap <= %d, got %s"
                         % (what, MAX_ANCHORS, tuple(keys.shape)))
    B, cap = int(keys.shape[0]), int(keys.shape[1])
    keys = keys.contiguous()
    n_anchors = _args.lengths(anchors.n_anchors, B, dev, what, "anchors.n_anchors", on_gpu=True)
    lengths = _args.lengths(anchors.lengths, B, dev, what, "anchors.lengths", on_gpu=True)
    max_len = _int_in(what, "anchors.max_len", anchors.max_len, 1, MAX_READ_LEN)
    lib = _lib.load()
    with torch.cuda.device(dev):
        result = torch.empty(B, 8, dtype=torch.int32, device=dev)
        f, pred = (torch.empty(B, cap, dtype=torch.int32, device=dev) for _ in range(2)) if want_pred else (None, None)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.wn_chain(_p(keys), _p(n_anchors), _p(lengths), B, max_len, cap, anchors.k, args[0], args[1], args[2], args[3], args[4],
                                _p(result), _p(f), _p(pred), _p(bad), _stream()), "wn_chain")
        _args.note_bad(bad, lambda n, L=max_len, cap=cap: "wavenet_speech_amd.%s: %d read(s) with a length outside [0, %d] or an anchor "
                       "count outside [0, %d] (left unmapped)" % (what, n, L, cap))
    return ReadMapping(*(result[:, i] for i in range(8)), f, pred, anchors=anchors)


def chain_anchors(anchors, h=64, max_dist=5000, bandwidth=500, gap_base=2, gap_log=8, want_pred=False):
    """Chain the anchors of every read, each strand on its own: anchor i starts a chain at 16 k or extends one
    of its h (<= 1024) predecessors j in (r, q') order with 0 < dr, dq <= max_dist and |dr - dq| <= bandwidth at f(j) + 16 min(dr, dq, k)
    - gap(|dr - dq|), gap(0) = 0, gap(d) = gap_base d + gap_log floor(log2 d).  A fresh start beats an extension of equal score, and
    of equal extensions the nearest predecessor wins: minimap2's rules.  The best anchor of both strands (ties to the forward strand,
    then to the first in order) gives the mapping; runner_up is the best score on any other chain.  Not built: minimap2's max_skip
    heuristic, secondary chains beyond the runner-up score, base-level extension.  Returns ReadMapping."""
    what = "chain_anchors"
    return _chain(what, anchors, _chain_args(what, h, max_dist, bandwidth, gap_base, gap_log), bool(want_pred))


def map_reads(labels, lengths, index, max_occ=8, anchors_per_read=4096, h=64, max_dist=5000, bandwidth=500, gap_base=2, gap_log=8,
              want_pred=False, chunk=None):
    """seed_anchors, then chain_anchors: labels [B, L] int32 or int64 GPU rows (L <= 65535) with lengths [B] -- what
    ctc_greedy_decode returned, a beam of ctc_beam_decode, the rows of trim_reads -- against a ReadIndex on the same device.  No host
    synchronisation: with fixed shapes the call captures into a graph.  Returns ReadMapping; its .anchors holds the sorted anchor
    rows, n_minimizers and truncated.  A read whose length lies outside [0, L] is left unmapped and reported through
    check_device_flags()."""
    what = "map_reads"
    max_occ, cap = _seed_args(what, index, max_occ, anchors_per_read)
    args = _chain_args(what, h, max_dist, bandwidth, gap_base, gap_log)
    chunk = _chunk_arg(what, chunk)
    return _chain(what, _seed(what, labels, lengths, index, max_occ, cap, chunk, report=False), args, bool(want_pred))


def paf_records(names, lengths, mapping, ref_name, alignment=None, ref_length=None, cigars=None):
    """host helper: one PAF line per MAPPED read (unmapped reads have none, as with minimap2), "\\n"-terminated: query name, length,
    start, end, strand, reference name, length, start, end, matches, alignment length, mapping quality.  Columns 10 and 11 come from
    a PairwiseAlignment of the mapped stretches (matches, length) when one is given; otherwise they are an APPROXIMATION:
    min(n_anchors k, query span) and the longer of the two spans.  ref_length: needed only for a mapping without a reference.
    cigars: the CigarRows of cigar_runs (sam.py) for the same reads; a line whose row was written then gains NM:i: and cg:Z:, the
    runs without the soft clips (PAF has none); a row with used < 0 raises.  Without it every line is as before."""
    what = "paf_records"
    names = [str(n) for n in names]
    ns = [int(n) for n in torch.as_tensor(lengths).cpu().reshape(-1).tolist()]
    if not isinstance(mapping, ReadMapping):
        raise ValueError("wavenet_speech_amd.%s: mapping must be a ReadMapping" % what)
    if ref_length is None:
        if mapping.reference is None:
            raise ValueError("wavenet_speech_amd.%s: ref_length is needed for a mapping without a reference" % what)
        ref_length = mapping.reference.R
    cols = [t.cpu().tolist() for t in (mapping.strand, mapping.ref_start, mapping.ref_end, mapping.query_start, mapping.query_end,
                                       mapping.n_anchors)]
    mapq = mapping.mapq().cpu().tolist()
    if not (len(names) == len(ns) == len(cols[0])):
        raise ValueError("wavenet_speech_amd.%s: %d names, %d lengths, %d mapped rows" % (what, len(names), len(ns), len(cols[0])))
    if alignment is not None:
        nmatch, alen = alignment.matches.cpu().tolist(), alignment.length.cpu().tolist()
        if len(nmatch) != len(names):
            raise ValueError("wavenet_speech_amd.%s: the alignment holds %d rows for %d reads" % (what, len(nmatch), len(names)))
    tags = [""] * len(names)
    if cigars is not None:
        from . import sam
        runs, rows = sam._host_rows(cigars, what)
        if len(runs) != len(names):
            raise ValueError("wavenet_speech_amd.%s: the cigars hold %d rows for %d reads" % (what, len(runs), len(names)))
        if any(u < 0 and s >= 0 for u, s in zip(rows[6], cols[0])):
            raise ValueError("wavenet_speech_amd.%s: a mapped read has no CIGAR (used < 0)" % what)
        tags = ["\tNM:i:%d\tcg:Z:%s" % (nm, sam._cigar_text([r for r in run if r[1] != 4], cigars.eqx)) if u == 1 else ""
                for run, nm, u in zip(runs, rows[5], rows[6])]
    out = []
    for b, name in enumerate(names):
        s, r0, r1, q0, q1, na = (c[b] for c in cols)
        if s < 0:
            continue
        if alignment is not None:
            m, a = int(nmatch[b]), int(alen[b])
        else:
            m, a = min(na * mapping.k, q1 - q0), max(q1 - q0, r1 - r0)
        out.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d%s\n" % (name, ns[b], q0, q1, "+-"[s], ref_name, int(ref_length), r0, r1, m, a,
                                                                        int(math.floor(mapq[b] + 0.5)), tags[b]))
    return out
