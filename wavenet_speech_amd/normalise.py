"""
Read normalisation on the device: exact per-read order statistics of ragged reads, and from them the two numbers per read
that Basecaller.__call__ and chunk_gather apply to raw samples, x = (raw + shift) * scale.

    scale, shift = read_normalisation(signal, signal_lengths)            # median / MAD
    out = bc(signal, signal_lengths, scale=scale, shift=shift)           # or simply bc(signal, signal_lengths, normalise="medmad")

signal is [B, Lpad] or [B, 1, Lpad], fp32 or int16 DAC counts, read b in its first signal_lengths[b] samples; signal_lengths is
a DEVICE tensor and is never read back.  Everything is a selection (csrc/wn_select.hip: a most-significant-digit radix select
with integer histograms), not a sort: exact, bitwise reproducible, a fixed number of launches, capturable into a HIP graph.

Order: fp32 values are ordered by their bits, sign-corrected: -0.0 sorts directly below +0.0 (they compare equal, either may
be returned), a NaN with a clear sign bit sorts above +inf as in torch.sort, one with the sign bit set below -inf.
A rank outside [0, n), every rank of an empty read and a read whose length is negative or above Lpad are refused on the device:
their result is 0.0 and they are counted; the count raises a RuntimeError through the package's device flags (_flags.WATCH)
unless the caller passes its own `bad` counter.  There is no CPU fallback: CPU tensors raise.
"""
import torch

from . import _args, _flags, _lib
from ._args import _p, _stream

TILE = 8192                 # samples per workgroup of a pass (kSelTile in csrc/wn_select.hip)
MAX_RANKS = 8               # K of one wn_read_select call
MAD_TO_SD = 1.4826          # the MAD of a normal distribution is sd / 1.4826


def _signal2d(signal, what):
    return _args.signal_rows(signal, what, error=TypeError, dense=True)      # dense rows: the row length is the reads' capacity


def _lengths(signal_lengths, B, device, what):
    return _args.lengths(signal_lengths, B, device, what, "signal_lengths", on_gpu=True)       # never read back, never uploaded


def select_workspace(batch, K, dtype, has_center, device):
    """the workspace of one read_order_statistics call (uint8 tensor): allocate it once to keep a captured graph's memory fixed"""
    n = int(_lib.load().wn_read_select_workspace_bytes(int(batch), int(K), int(dtype == torch.int16), int(bool(has_center))))
    if n == 0:
        raise ValueError("wavenet_speech_amd.select_workspace: unsupported shape: batch = %d (1..65535), K = %d (1..%d)"
                         % (batch, K, MAX_RANKS))
    return torch.empty(n, dtype=torch.uint8, device=device)


def read_order_statistics(signal, signal_lengths, ranks, center=None, bad=None, workspace=None):
    """csrc/wn_select.hip, wn_read_select: out [B, K] fp32, out[b][k] = the ranks[b][k]-th smallest (0-based) of read b's first
    signal_lengths[b] samples; with center [B] fp32, of the deviations |float(x) - center[b]| computed in fp32.
    ranks [B, K] integers on the device, K <= 8.  bad: [1] int32 device counter of refused (b, k) entries, accumulated into and
    left to the caller; None: counted internally and raised as a RuntimeError.  workspace: from select_workspace, or None."""
    what = "read_order_statistics"
    signal = _signal2d(signal, what)
    B, ld = int(signal.shape[0]), int(signal.shape[1])
    dev = signal.device
    len_d = _lengths(signal_lengths, B, dev, what)
    ranks = _args.gpu_tensor(ranks, what, "ranks")
    if ranks.is_floating_point() or ranks.dim() != 2 or ranks.shape[0] != B or not 1 <= ranks.shape[1] <= MAX_RANKS:
        raise ValueError("wavenet_speech_amd.%s: ranks must be integers of shape (%d, K), 1 <= K <= %d, got %s %s"
                         % (what, B, MAX_RANKS, ranks.dtype, tuple(ranks.shape)))
    K = int(ranks.shape[1])
    ranks = ranks.to(device=dev, dtype=torch.int32).contiguous()
    if center is not None:
        if not isinstance(center, torch.Tensor) or not center.is_cuda or center.shape != (B,):
            raise ValueError("wavenet_speech_amd.%s: center must be a GPU tensor of shape (%d,)" % (what, B))
        center = center.detach().to(device=dev, dtype=torch.float32).contiguous()
    own_bad = bad is None
    with torch.cuda.device(dev):
        if own_bad:
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
        elif not isinstance(bad, torch.Tensor) or not bad.is_cuda or bad.dtype != torch.int32 or bad.numel() != 1:
            raise ValueError("wavenet_speech_amd.%s: bad must be an int32 GPU tensor of one element" % what)
        if workspace is None:
            workspace = select_workspace(B, K, signal.dtype, center is not None, dev)
        elif not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.dtype != torch.uint8 \
                or not workspace.is_contiguous():
            raise ValueError("wavenet_speech_amd.%s: workspace must be a contiguous uint8 GPU tensor (select_workspace)" % what)
        out = torch.empty(B, K, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().wn_read_select(_p(signal), int(signal.dtype == torch.int16), B, ld, _p(len_d), _p(ranks), K, _p(center),
                                              _p(out), _p(workspace), int(workspace.numel()), _p(bad), _stream()), "wn_read_select")
        if own_bad:
            _note(bad, what)
    return out


def _note(bad, what):
    _flags.WATCH.note(bad, lambda n: "wavenet_speech_amd.%s: %d order statistic(s) refused by the selection kernels (a read length "
                      "below 0 or above the row length, an empty read, or a rank outside its read)" % (what, n), at_once=True)


def _midpoint(pair):
    return (pair[:, 0] + pair[:, 1]) * 0.5          # two fp32 operations, each rounded: fl(fl(a + b) * 0.5)


def _middle_ranks(len_d):
    n = len_d.to(torch.int64)
    return torch.stack((torch.div(n - 1, 2, rounding_mode="floor"), torch.div(n, 2, rounding_mode="floor")), dim=1).to(torch.int32)


def read_med_mad(signal, signal_lengths, bad=None, workspaces=None):
    """(med [B], mad [B]) fp32 of every read: with a, b the order statistics at ranks (n - 1) // 2 and n // 2, med = fl(fl(a + b)
    * 0.5), and mad the same midpoint over the deviations |x - med| (fp32).  Two selections with K = 2.  For int16 reads both are
    exact (multiples of 0.25).  workspaces: a pair (select_workspace(B, 2, dtype, False, dev), select_workspace(B, 2, dtype, True,
    dev)) to reuse, or None.  bad: as read_order_statistics (one counter for both selections)."""
    what = "read_med_mad"
    signal = _signal2d(signal, what)
    len_d = _lengths(signal_lengths, int(signal.shape[0]), signal.device, what)
    own_bad = bad is None
    ws = workspaces if workspaces is not None else (None, None)
    with torch.cuda.device(signal.device):
        if own_bad:
            bad = torch.zeros(1, dtype=torch.int32, device=signal.device)
        ranks = _middle_ranks(len_d)
        med = _midpoint(read_order_statistics(signal, len_d, ranks, bad=bad, workspace=ws[0]))
        mad = _midpoint(read_order_statistics(signal, len_d, ranks, center=med, bad=bad, workspace=ws[1]))
        if own_bad:
            _note(bad, what)
    return med, mad


def _quantile_positions(len_d, q):
    """pos = q (n - 1) in fp64, lo = floor(pos), hi = ceil(pos): [B, Q] each.  hi = lo + 1 wherever pos has a fraction, and lo where
    it has none -- there the weight of v_hi is 0 and "higher" / "midpoint" are the element at pos itself, as in numpy."""
    qd = torch.tensor(q, dtype=torch.float64, device=len_d.device)
    pos = qd[None, :] * (len_d.to(torch.float64) - 1.0)[:, None]
    lo = torch.floor(pos)
    hi = torch.ceil(pos)
    return pos, lo, hi


def read_quantiles(signal, signal_lengths, q, interpolation="linear", bad=None, workspace=None):
    """[B, len(q)] fp32: the quantiles q (floats in [0, 1], at most 4) of every read, numpy's definition: pos = q (n - 1) in fp64,
    lo = floor(pos), hi = ceil(pos) (lo + 1 capped at n - 1, wherever it matters), v the order statistics at lo and hi.
    "lower" v_lo, "higher" v_hi, "midpoint" fl(fl(v_lo + v_hi) * 0.5): exact selections; "linear" v_lo + (v_hi - v_lo) (pos - lo)
    evaluated in fp64 and rounded once to fp32.  One selection with K = 2 len(q)."""
    what = "read_quantiles"
    if interpolation not in ("linear", "lower", "higher", "midpoint"):
        raise ValueError("wavenet_speech_amd.%s: interpolation must be 'linear', 'lower', 'higher' or 'midpoint', got %r"
                         % (what, interpolation))
    q = [float(v) for v in q]
    if not 1 <= len(q) <= MAX_RANKS // 2 or any(not 0.0 <= v <= 1.0 for v in q):
        raise ValueError("wavenet_speech_amd.%s: q must hold 1 to %d values in [0, 1], got %r" % (what, MAX_RANKS // 2, q))
    signal = _signal2d(signal, what)
    len_d = _lengths(signal_lengths, int(signal.shape[0]), signal.device, what)
    Q = len(q)
    with torch.cuda.device(signal.device):
        pos, lo, hi = _quantile_positions(len_d, q)
        ranks = torch.cat((lo, hi), dim=1).to(torch.int32)                       # an empty read: pos < 0, refused on the device
        v = read_order_statistics(signal, len_d, ranks, bad=bad, workspace=workspace)
        v_lo, v_hi = v[:, :Q], v[:, Q:]
        if interpolation == "lower":
            return v_lo.contiguous()
        if interpolation == "higher":
            return v_hi.contiguous()
        if interpolation == "midpoint":
            return (v_lo + v_hi) * 0.5
        a, b = v_lo.to(torch.float64), v_hi.to(torch.float64)
        return (a + (b - a) * (pos - lo)).to(torch.float32)


def read_normalisation(signal, signal_lengths, method="medmad", q=(0.2, 0.9), factor=1.0, min_spread=1e-6, bad=None):
    """(scale [B], shift [B]) fp32, the two tensors Basecaller.__call__ and chunk_gather take: x = (raw + shift) * scale.
    "medmad": shift = -med, scale = 1 / (1.4826f * mad) in fp32, 1 where mad == 0 (a constant read).
    "quantile": with (a, b) the "linear" quantiles q = (q_lo, q_hi): shift = -fl(fl(a + b) * 0.5), scale = 1 / max((b - a) * factor,
    min_spread) in fp32."""
    what = "read_normalisation"
    if method == "medmad":
        med, mad = read_med_mad(signal, signal_lengths, bad=bad)
        spread = mad * MAD_TO_SD                    # the Python scalar enters as fp32: 1.4826f
        scale = torch.where(mad == 0, torch.ones_like(mad), 1.0 / spread)
        return scale, -med
    if method == "quantile":
        if len(q) != 2 or not float(q[0]) < float(q[1]):
            raise ValueError("wavenet_speech_amd.%s: q must be (q_lo, q_hi) with q_lo < q_hi, got %r" % (what, (q,)))
        if not float(factor) > 0.0 or not float(min_spread) > 0.0:
            raise ValueError("wavenet_speech_amd.%s: factor and min_spread must be positive, got %r, %r" % (what, factor, min_spread))
        v = read_quantiles(signal, signal_lengths, q, bad=bad)
        spread = torch.clamp((v[:, 1] - v[:, 0]) * float(factor), min=float(min_spread))
        return 1.0 / spread, -_midpoint(v)
    raise ValueError("wavenet_speech_amd.%s: method must be 'medmad' or 'quantile', got %r" % (what, method))
