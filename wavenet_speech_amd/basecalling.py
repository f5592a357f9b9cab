"""
Whole-read basecalling: a trained RawCTCNet applied to reads of any length through ONE fixed forward shape.

The network is a stride-1 convolutional stack with a finite receptive field, so a read is cut into chunks of `chunk` samples
that overlap by that field, all chunks run as fixed-shape [batch, 1, chunk] micro-batches, every chunk keeps only the frames
whose receptive field lay inside it, and the kept frames are put back together.  Cropping is exact: there is no seam error
and nothing is averaged.

    bc = Basecaller(model, chunk=4096, batch=32, graph=True)
    out = bc(signal, signal_lengths, decode="greedy")     # signal [B, 1, Lpad] or [B, Lpad], fp32 or int16 DAC counts
    out = bc(raw_int16, signal_lengths, normalise="medmad")             # per-read median / MAD on the device (normalise.py)
    out.logits, out.frame_lengths, out.labels, out.label_lengths
    q = bc.qualities(out)                                 # Phred quality per base, mean error per read (decoding.py)
    prof = bc.calibrate(out, truth, truth_lengths)        # calls against known truth: calibration tables, error profile

What a basecall is: the logits of read b (n samples) are the T_b = n + feature_kwidth - 1 frames of the model's forward on the
read FOLLOWED BY ZEROS, model(F.pad(read, (0, p)))[..., :T_b] for any p >= right -- what training on zero-padded ragged
batches (synthetic.ragged_reads) shows the model for every read but the longest of a batch.  This differs from model(read)
alone in the last `right` frames at most: there the convolutions' own padding (zeros at the FEATURE level) takes the place of
the features of zero samples, and those are not the same thing.  Causal models have right = 0 and no such difference.

Gather (raw samples -> chunk rows) and stitch (kept frames -> [B, C, Tmax]) are HIP kernels (csrc/wn_chunk.hip); the plan is
host arithmetic, so the read lengths are needed on the host: lengths given as a device tensor cost one read-back per call,
like the max() of ragged_reads(pad_to=None).  There is no CPU fallback: CPU tensors raise.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _args, _flags, _lib, series
from ._args import _p, _stream
from .decoding import ctc_base_qualities, ctc_beam_decode, ctc_greedy_decode, pairwise_align, quality_profile
from .modules.block import freeze_for_inference
from .modules.raw_ctcnet import RawCTCNet
from .normalise import read_normalisation

PLAN_INTS = 5                       # (read, s0, u_lo, t0, count)
MAX_DIM = 2 ** 31 - 1024            # ld, chunk and frame counts of the C ABI stay below this

ChunkPlan = namedtuple("ChunkPlan", "rows frame_lengths chunks_per_read")
ChunkPlan.__doc__ = """rows [N, 5] int32 (read, s0, u_lo, t0, count), reads in order: the chunk holds samples [s0, s0 + chunk)
of `read`, and its frames [u_lo, u_lo + count) are frames [t0, t0 + count) of the read.  frame_lengths [B] int32 = n +
feature_kwidth - 1.  chunks_per_read [B] int32.  All host tensors."""

Basecalls = namedtuple("Basecalls", "logits frame_lengths labels label_lengths frames scores")
Basecalls.__doc__ = """logits [B, C, Tmax] fp32 (the model's own output: probabilities if it has softmax=True), exactly 0 past
frame_lengths [B] int32; labels / label_lengths / frames / scores in the shapes of ctc_greedy_decode (scores None) or
ctc_beam_decode, None without decode.  All on the device."""


def receptive_field(model):
    """(left, right) in samples: output frame t of `model` (a RawCTCNet) depends on samples [t - left, t + right] and on no
    other.  Every residual block (k, d), the input block first, reaches max(0, -min(offs)) to the left and max(0, max(offs))
    to the right, offs = tap_offsets(k, d, causal); the feature conv (padding = feature_kwidth - 1) adds feature_kwidth - 1
    to the left only.  Host arithmetic on the model's attributes."""
    if not isinstance(model, RawCTCNet):
        raise TypeError("receptive_field: needs a RawCTCNet, got %s" % type(model).__name__)
    if model.positions:
        raise ValueError("receptive_field: positions=True mixes the absolute frame index into every frame; a chunk cannot "
                         "reproduce it")
    left, right = model.feature_kwidth - 1, 0
    for k, d in [(model.input_kernel_size, model.input_dilation)] + [(k, d) for (_ci, _co, k, d) in model.layers]:
        offs = _lib.tap_offsets(int(k), int(d), bool(model.causal))
        left += max(0, -min(offs))
        right += max(0, max(offs))
    return left, right


def chunk_plan(signal_lengths, chunk, left, right, feature_kwidth, capacity=None):
    """The chunks of every read (host): ChunkPlan.  See _plan for the arithmetic.  signal_lengths: [B] integers (a device tensor
    is read back).  capacity: the row length the reads are stored in, if known.  ValueError on a length < 1 or above the
    capacity, chunk < left + right + 1 or chunk % 4 != 0 (the gather kernel writes rows 16 bytes at a time)."""
    return _plan(signal_lengths, chunk, left, right, feature_kwidth, capacity, 4)


def _plan(signal_lengths, chunk, left, right, feature_kwidth, capacity, multiple):
    """The chunks of every read (host).  Read b of n samples has T = n + feature_kwidth - 1 frames.  Chunk 0 starts at sample
    0 and keeps frames [0, min(T, chunk - right)); every later chunk with first kept frame t0 starts at sample t0 - left and
    keeps its local frames [left, chunk - right), i.e. read frames [t0, min(T, t0 - left + chunk - right)).  So a read has 1
    chunk if T <= chunk - right, else 1 + ceil((T - (chunk - right)) / (chunk - left - right)).
    multiple: what chunk must be a multiple of; the arithmetic itself holds for any chunk."""
    chunk, left, right, fk = int(chunk), int(left), int(right), int(feature_kwidth)
    if left < 0 or right < 0 or fk < 1:
        raise ValueError("chunk_plan: need left >= 0, right >= 0 and feature_kwidth >= 1, got %d, %d, %d" % (left, right, fk))
    if chunk < left + right + 1:
        raise ValueError("chunk_plan: chunk = %d cannot hold the receptive field: need at least left + right + 1 = %d"
                         % (chunk, left + right + 1))
    if multiple < 1 or chunk % multiple != 0:
        raise ValueError("chunk_plan: chunk must be a multiple of %d (rows are written 16 bytes at a time), got %d" % (multiple, chunk))
    if chunk >= MAX_DIM:
        raise ValueError("chunk_plan: chunk must be below %d, got %d" % (MAX_DIM, chunk))
    lengths = torch.as_tensor(signal_lengths)
    if lengths.is_floating_point() or lengths.dtype == torch.bool or lengths.dim() != 1 or lengths.numel() < 1:
        raise ValueError("chunk_plan: signal_lengths must be integers of shape (B,), got %s %s" % (lengths.dtype, tuple(lengths.shape)))
    n = lengths.detach().cpu().numpy().astype(np.int64)
    cap = MAX_DIM - fk if capacity is None else min(int(capacity), MAX_DIM - fk)
    if int(n.min()) < 1 or int(n.max()) > cap:
        raise ValueError("chunk_plan: every read needs between 1 and %d samples, got lengths from %d to %d"
                         % (cap, int(n.min()), int(n.max())))
    T = n + (fk - 1)
    first, step = chunk - right, chunk - left - right
    per_read = 1 + np.maximum(0, -((first - T) // step))                # 1 + ceil((T - first) / step), never below 1
    total = int(per_read.sum())
    rows = np.zeros((total, PLAN_INTS), dtype=np.int64)
    read = np.repeat(np.arange(len(n)), per_read)
    j = np.arange(total) - np.repeat(np.cumsum(per_read) - per_read, per_read)          # index of the chunk inside its read
    t0 = np.where(j == 0, 0, first + (j - 1) * step)
    s0 = np.where(j == 0, 0, t0 - left)
    rows[:, 0] = read
    rows[:, 1] = s0
    rows[:, 2] = np.where(j == 0, 0, left)
    rows[:, 3] = t0
    rows[:, 4] = np.minimum(T[read], s0 + first) - t0
    return ChunkPlan(torch.from_numpy(rows.astype(np.int32)), torch.from_numpy(T.astype(np.int32)),
                     torch.from_numpy(per_read.astype(np.int32)))


def _need(t, name, dtypes, what, dense=True):
    _args.gpu_tensor(t, what, name, dtypes, TypeError)
    if dense and not t.is_contiguous():
        raise ValueError("wavenet_speech_amd.%s: %s must be contiguous" % (what, name))


def chunk_gather(signal, signal_lengths, plan, chunk, out, scale=None, shift=None, bad=None):
    """csrc/wn_chunk.hip, wn_chunk_gather: out[n] = the `chunk` samples of plan row n.  Device tensors: signal [B, ld] fp32 or
    int16 with dense rows (the row length is the capacity the kernel holds signal_lengths to), signal_lengths [B] int32, plan
    [N, 5] int32, out [N, chunk] fp32, scale / shift [B] fp32 or None, bad [1] int32 or None; all contiguous."""
    what = "chunk_gather"
    _need(signal, "signal", (torch.float32, torch.int16), what)
    _need(signal_lengths, "signal_lengths", (torch.int32,), what)
    _need(plan, "plan", (torch.int32,), what)
    _need(out, "out", (torch.float32,), what)
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _need(t, name, (torch.float32,), what)
    if bad is not None:
        _need(bad, "bad", (torch.int32,), what)
    if signal.dim() != 2 or plan.dim() != 2 or plan.shape[1] != PLAN_INTS or tuple(out.shape) != (plan.shape[0], int(chunk)):
        raise ValueError("wavenet_speech_amd.%s: need signal [B, ld], plan [N, %d] and out [N, chunk], got %s, %s, %s"
                         % (what, PLAN_INTS, tuple(signal.shape), tuple(plan.shape), tuple(out.shape)))
    B, ld = int(signal.shape[0]), int(signal.shape[1])
    if signal_lengths.shape != (B,) or any(t is not None and t.shape != (B,) for t in (scale, shift)):
        raise ValueError("wavenet_speech_amd.%s: signal_lengths, scale and shift must have shape (%d,)" % (what, B))
    _lib.check(_lib.load().wn_chunk_gather(_p(signal), int(signal.dtype == torch.int16), B, ld, _p(signal_lengths), _p(scale),
                                           _p(shift), _p(plan), int(plan.shape[0]), int(chunk), _p(out), _p(bad), _stream()),
               "wn_chunk_gather")


def chunk_stitch(y, plan, out, frame_lengths, bad=None):
    """csrc/wn_chunk.hip, wn_chunk_stitch: the kept frames of y [N, C, Ty] fp32 (any non-negative strides) into out [B, C, Tmax]
    fp32 (zero-filled by the caller, unit stride in time); plan [N, 5] int32 and frame_lengths [B] int32 contiguous."""
    what = "chunk_stitch"
    _need(y, "y", (torch.float32,), what, dense=False)
    _need(out, "out", (torch.float32,), what, dense=False)
    _need(plan, "plan", (torch.int32,), what)
    _need(frame_lengths, "frame_lengths", (torch.int32,), what)
    if bad is not None:
        _need(bad, "bad", (torch.int32,), what)
    if y.dim() != 3 or out.dim() != 3 or tuple(plan.shape) != (y.shape[0], PLAN_INTS) or out.shape[1] != y.shape[1] \
            or frame_lengths.shape != (out.shape[0],) or out.stride(2) != 1:
        raise ValueError("wavenet_speech_amd.%s: need y [N, C, Ty], plan [N, %d], out [B, C, Tmax] with unit stride in time and "
                         "frame_lengths [B], got %s, %s, %s, %s" % (what, PLAN_INTS, tuple(y.shape), tuple(plan.shape), tuple(out.shape),
                                                                    tuple(frame_lengths.shape)))
    _lib.check(_lib.load().wn_chunk_stitch(_p(y), y.stride(0), y.stride(1), y.stride(2), int(y.shape[2]), _p(plan),
                                           int(plan.shape[0]), int(y.shape[1]), int(out.shape[0]), _p(out), out.stride(0),
                                           out.stride(1), int(out.shape[2]), _p(frame_lengths), _p(bad), _stream()),
               "wn_chunk_stitch")


class Basecaller(object):
    """model: a RawCTCNet on the device, in the precision set_precision selected.  Construction switches it to eval, calls
    freeze_for_inference (packed weights are kept across forwards) and fixes the forward shape [batch, 1, chunk].
    graph=True: the no-grad forward of that static buffer is captured once into a HIP graph and replayed per micro-batch (the
    same kernels through the same C ABI: bitwise the eager forward); gather and stitch stay outside it, their plan changes
    with every call.  The capture is made again when a parameter was updated since."""

    def __init__(self, model, chunk=4096, batch=32, graph=False):
        self.left, self.right = receptive_field(model)
        self.chunk, self.batch = int(chunk), int(batch)
        if self.batch < 1 or self.batch > 65535:
            raise ValueError("Basecaller: batch must be in [1, 65535], got %d" % self.batch)
        chunk_plan([1], self.chunk, self.left, self.right, model.feature_kwidth)         # raises on a chunk that cannot work
        p = next(model.parameters())
        if not p.is_cuda:
            raise RuntimeError("wavenet_speech_amd.Basecaller: the model must be on a GPU (there is no CPU fallback)")
        self.device = p.device
        self.model = model.eval()
        freeze_for_inference(model)
        self.x = torch.zeros(self.batch, 1, self.chunk, dtype=torch.float32, device=self.device)
        self.graph = None
        self._want_graph = bool(graph)
        self._captured_key = None
        if self._want_graph:
            with torch.cuda.device(self.device):
                self._capture()

    @property
    def efficiency(self):
        """kept frames per computed sample of a long read: (chunk - left - right) / chunk"""
        return (self.chunk - self.left - self.right) / float(self.chunk)

    def _param_key(self):
        return tuple((id(p), p._version, p.data_ptr()) for p in self.model.parameters()) + (self.model.stack_state.precision,)

    def _forward(self):
        with torch.no_grad():
            return self.model(self.x)          # dense fp32 in every precision mode

    def _capture(self):
        """as graphs.GraphedStep: warm-up on the capture stream (the series pool, the allocator and the packed weights reach
        their steady state), pooled buffers held for the life of the graph, torch's graph-private pool for the rest"""
        dev = self.device
        self.stream = torch.cuda.Stream(device=dev)
        self.graph = torch.cuda.CUDAGraph()
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            for _ in range(2):
                self._forward()
            torch.cuda.current_stream().synchronize()
            # what the captured launches address besides pooled buffers: the packed weights of the frozen model
            self._packed = dict(self.model.stack_state.cache.packed), self.model.stack_state.folded
            seen = len(_flags.WATCH.captured)
            self.buffers = []
            series.POOL.hold = self.buffers
            try:
                with torch.cuda.graph(self.graph, stream=self.stream):
                    self.y = self._forward()
            finally:
                series.POOL.hold = None
            self._flags = _flags.WATCH.captured[seen:]          # device flags of the captured forward (fp16 overflow)
            del _flags.WATCH.captured[seen:]                    # read here after every replay, not by later unrelated checks
            self._raised = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in self._flags]
        torch.cuda.current_stream(dev).wait_stream(self.stream)
        self._captured_key = self._param_key()

    def _replay(self):
        self.graph.replay()
        for acc, (flag, _msg) in zip(self._raised, self._flags):    # every replay zeroes its flags: sum them before the next
            acc.add_(flag)
        return self.y

    def __call__(self, signal, signal_lengths, scale=None, shift=None, decode=None, beam_width=8, want_logits=True, normalise=None):
        """normalise: None (scale / shift as given, or none), "medmad" or "quantile" (normalise.read_normalisation with its
        defaults), or a callable (signal [B, Lpad], lengths [B] int32 on the device) -> (scale, shift): computed on the device
        before the first gather.  Not together with scale or shift."""
        what = "wavenet_speech_amd.Basecaller"
        if normalise is not None:
            if scale is not None or shift is not None:
                raise ValueError("%s: give either normalise or scale / shift, not both" % what)
            if not callable(normalise) and normalise not in ("medmad", "quantile"):
                raise ValueError("%s: normalise must be None, 'medmad', 'quantile' or a callable, got %r" % (what, normalise))
        if decode not in (None, "greedy", "beam"):
            raise ValueError("%s: decode must be None, 'greedy' or 'beam', got %r" % (what, decode))
        if not isinstance(signal, torch.Tensor) or not signal.is_cuda:
            raise RuntimeError("%s: signal must be a GPU tensor (there is no CPU fallback)" % what)
        if signal.device != self.device:
            raise RuntimeError("%s: signal is on %s, the model on %s" % (what, signal.device, self.device))
        if signal.dim() == 3 and signal.shape[1] == 1:
            signal = signal[:, 0]
        if signal.dim() != 2 or signal.shape[0] < 1 or signal.shape[1] < 1:
            raise ValueError("%s: signal must be [B, 1, Lpad] or [B, Lpad], got shape %s" % (what, tuple(signal.shape)))
        if signal.dtype not in (torch.float32, torch.int16):
            raise TypeError("%s: signal must be float32 or int16, got %s" % (what, signal.dtype))
        signal = signal.detach()
        B, Lpad = int(signal.shape[0]), int(signal.shape[1])
        if not signal.is_contiguous():
            signal = signal.contiguous()          # dense rows: the row length is the capacity the gather checks lengths against
        dev = self.device
        affine = []
        for name, v in (("scale", scale), ("shift", shift)):
            if v is not None:
                if not isinstance(v, torch.Tensor) or not v.is_cuda or v.shape != (B,):
                    raise ValueError("%s: %s must be a GPU tensor of shape (%d,)" % (what, name, B))
                v = v.detach().to(device=dev, dtype=torch.float32).contiguous()
            affine.append(v)
        scale, shift = affine
        lengths = torch.as_tensor(signal_lengths)
        if lengths.shape != (B,):
            raise ValueError("%s: signal_lengths must have shape (%d,), got %s" % (what, B, tuple(lengths.shape)))
        fk = self.model.feature_kwidth
        plan = chunk_plan(lengths, self.chunk, self.left, self.right, fk, capacity=Lpad)         # host; one read-back if on the device
        n_live = int(plan.rows.shape[0])
        n_all = -(-n_live // self.batch) * self.batch
        rows = torch.zeros(n_all, PLAN_INTS, dtype=torch.int32)             # dead chunks (count 0) fill the last micro-batch
        rows[:n_live] = plan.rows
        if self.model.training or not self.model.stack_state.cache.frozen:       # train() or set_precision() since construction
            freeze_for_inference(self.model.eval())
        with torch.cuda.device(dev):
            if self._want_graph and self._captured_key != self._param_key():
                self._capture()                                             # a parameter changed: the graph holds stale packed weights
            rows_d = rows.to(dev, non_blocking=False)
            len_d = lengths.to(device=dev, dtype=torch.int32).contiguous()
            if normalise is not None:
                scale, shift = normalise(signal, len_d) if callable(normalise) else read_normalisation(signal, len_d, method=normalise)
                for name, v in (("scale", scale), ("shift", shift)):
                    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.shape != (B,):
                        raise ValueError("%s: normalise must return (scale, shift), GPU tensors of shape (%d,)" % (what, B))
                scale = scale.detach().to(device=dev, dtype=torch.float32).contiguous()
                shift = shift.detach().to(device=dev, dtype=torch.float32).contiguous()
            frame_lengths = plan.frame_lengths.to(dev)
            Tmax = int(plan.frame_lengths.max())
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            x2 = self.x.view(self.batch, self.chunk)
            logits = None
            if self.graph is not None:
                for acc in self._raised:
                    acc.zero_()
            for m0 in range(0, n_all, self.batch):
                part = rows_d[m0:m0 + self.batch]
                chunk_gather(signal, len_d, part, self.chunk, x2, scale, shift, bad)
                y = self._replay() if self.graph is not None else self._forward()
                if logits is None:
                    logits = torch.zeros(B, int(y.shape[1]), Tmax, dtype=torch.float32, device=dev)
                chunk_stitch(y, part, logits, frame_lengths, bad)
            if self.graph is not None:
                for acc, (_flag, msg) in zip(self._raised, self._flags):
                    _flags.WATCH.note(acc, msg, at_once=True)
            _flags.WATCH.note(bad, lambda n: "%s: %d plan row(s) refused by the gather / stitch kernels (lengths or plan out of "
                              "range)" % (what, n), at_once=True)
            labels = label_lengths = frames = scores = None
            if decode == "greedy":
                labels, label_lengths, frames = ctc_greedy_decode(logits, input_lengths=frame_lengths)
            elif decode == "beam":
                labels, label_lengths, scores, frames = ctc_beam_decode(logits, beam_width, input_lengths=frame_lengths,
                                                                        input="probs" if self.model.softmax else "logits")
        return Basecalls(logits if want_logits else None, frame_lengths, labels, label_lengths, frames, scores)

    def qualities(self, calls, **kw):
        """Per-base qualities of a decoded Basecalls (decoding.ctc_base_qualities, whose keyword arguments pass through: stat,
        qscale, qbias, blank): the labels of a greedy decode, or the best beam of a beam search, against the logits they were
        decoded from -- read as probabilities when the model applies its own softmax.  Returns BaseQualities."""
        what = "wavenet_speech_amd.Basecaller.qualities"
        if calls.logits is None:
            raise ValueError("%s: the Basecalls carry no logits (they were made with want_logits=False)" % what)
        if calls.labels is None:
            raise ValueError("%s: the Basecalls carry no labels (they were made without decode=)" % what)
        labels, lengths, frames = calls.labels, calls.label_lengths, calls.frames
        if labels.dim() == 3:                                         # beam search: [B, W, T], the best beam first
            labels, lengths, frames = labels[:, 0], lengths[:, 0], frames[:, 0]
        kw.setdefault("input", "probs" if self.model.softmax else "logits")
        return ctc_base_qualities(calls.logits, labels, lengths, frames, input_lengths=calls.frame_lengths, **kw)

    def calibrate(self, calls, truth, truth_lengths, into=None, **align_kw):
        """The calls of reads whose true bases are known, tabulated for fit_quality_calibration (decoding.quality_profile): the
        uncalibrated qualities and dwells of the calls (qscale=1, qbias=0), pairwise_align(truth, truth_lengths, the calls'
        labels, their lengths, **align_kw) -- needle's defaults unless align_kw says otherwise; return_ops=False raises -- and quality_profile over the
        classes of the logits.  into: the QualityProfile of earlier batches, accumulated in place.  Returns QualityProfile."""
        q = self.qualities(calls)
        labels, lengths = calls.labels, calls.label_lengths
        if labels.dim() == 3:
            labels, lengths = labels[:, 0], lengths[:, 0]
        if not align_kw.pop("return_ops", True):
            raise ValueError("wavenet_speech_amd.Basecaller.calibrate: the profile walks the ops; return_ops=False cannot be honoured")
        alignment = pairwise_align(truth, truth_lengths, labels, lengths, return_ops=True, **align_kw)
        return quality_profile(alignment, truth, truth_lengths, labels, lengths, qual=q.qual, dwell=q.dwell,
                               classes=int(calls.logits.shape[1]), into=into)
