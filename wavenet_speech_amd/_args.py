"""
The host-side argument layer of the C ABI callers: device pointers, the current stream, workspace buffers, and the checks and
preparations that the read tools (decoding, events, normalise, basecalling) apply to what a caller hands them.  Small functions;
every one raises "wavenet_speech_amd.<what>: <name> ..." so that the public function's name stays in the message.  Where two
callers differ in a rule (the exception class of a wrong dtype, which views are read in place), the rule is an argument.
"""
import ctypes

import torch

from . import _flags, _lib
from .series import Lease


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(x):
    """device pointer of a tensor / Lease / None"""
    if x is None:
        return None
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    if isinstance(x, Lease):
        return ctypes.c_void_p(x.ptr)
    return ctypes.c_void_p(x.data_ptr())


def _alloc_bytes(nbytes, what, device, status=-1):
    """uint8 device buffer of the size the library's query `what` returned; 0 is its refusal of the shape and raises `status`"""
    if nbytes == 0:
        _lib.check(status, what)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _names(dtypes):
    return " or ".join(str(d).replace("torch.", "") for d in dtypes)


def gpu_tensor(x, what, name, dtypes=None, error=ValueError, device=None):
    """x detached, if it is a GPU tensor (RuntimeError: there is no CPU fallback) of one of `dtypes` (else `error`, the class the
    public function has always raised: TypeError or ValueError) on `device` (ValueError); None skips a check"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("wavenet_speech_amd.%s: %s must be a GPU tensor (there is no CPU fallback)" % (what, name))
    if dtypes is not None and x.dtype not in dtypes:
        raise error("wavenet_speech_amd.%s: %s must be %s, got %s" % (what, name, _names(dtypes), x.dtype))
    if device is not None and x.device != device:
        raise ValueError("wavenet_speech_amd.%s: %s must be on %s" % (what, name, device))
    return x.detach()


def signal_rows(signal, what, error=ValueError, dense=False):
    """[B, L] or [B, 1, L] float32 / int16 samples as [B, L].  dense=False: a view is passed on by its row stride and copied only
    for a non-unit inner or a negative row stride; dense=True: the rows are made contiguous (their length is a capacity)."""
    signal = gpu_tensor(signal, what, "signal", (torch.float32, torch.int16), error)
    if signal.dim() == 3 and signal.shape[1] == 1:
        signal = signal[:, 0, :]
    if signal.dim() != 2 or signal.shape[0] < 1 or signal.shape[1] < 1:
        raise ValueError("wavenet_speech_amd.%s: signal must be [B, L] or [B, 1, L] with B, L >= 1, got %s" % (what, tuple(signal.shape)))
    if dense:
        return signal.contiguous()
    if signal.stride(1) != 1 and signal.shape[1] > 1 or signal.stride(0) < 0:
        signal = signal.contiguous()
    return signal


def int_rows(rows, what, name, B=None, shape="(B, n)", min_width=0, dtypes=(torch.int32, torch.int64), device=None, pad_empty=False,
             lone_column_in_place=True):
    """2-d integer rows for a kernel that reads them by their row stride: a GPU tensor of `dtypes` with B rows (None: any) and at
    least min_width columns -- `shape` is how the message writes that -- on `device` (None: any); int64 leaves as int32.
    pad_empty: rows without columns become one unused column (the C ABI wants a width of at least 1).  A unit inner stride is read
    in place (labels[:, 0] of a beam search); anything else is copied, except that a single column keeps whatever stride it has
    unless lone_column_in_place=False."""
    rows = gpu_tensor(rows, what, name)
    if rows.dtype not in dtypes or rows.dim() != 2 or (B is not None and rows.shape[0] != B) or rows.shape[1] < min_width:
        raise ValueError("wavenet_speech_amd.%s: %s must be %s of shape %s, got %s %s"
                         % (what, name, _names(dtypes), shape, rows.dtype, tuple(rows.shape)))
    if device is not None and rows.device != device:
        raise ValueError("wavenet_speech_amd.%s: %s must be on %s" % (what, name, device))
    if rows.dtype == torch.int64:
        rows = rows.to(torch.int32)                                  # on the device
    if pad_empty and rows.shape[1] == 0:
        rows = torch.zeros(rows.shape[0], 1, dtype=rows.dtype, device=rows.device)
    if rows.stride(1) != 1 and (rows.shape[1] > 1 or not lone_column_in_place) or rows.stride(0) < 0:
        rows = rows.contiguous()
    return rows


def lengths(x, B, device, what, name, on_gpu=False, flatten=False):
    """[B] lengths as contiguous int32 on `device`.  on_gpu: x must be a GPU tensor already (it is never uploaded); flatten: the
    lenient form of the event tools -- anything torch.as_tensor takes that holds B numbers, whatever its shape; otherwise integers
    of shape (B,), a tensor, an array or a list."""
    if on_gpu:
        gpu_tensor(x, what, name)
    x = torch.as_tensor(x)
    if flatten:
        x = x.to(device=device, dtype=torch.int32).reshape(-1).contiguous()
        if x.shape[0] != B:
            raise ValueError("wavenet_speech_amd.%s: %s must hold %d lengths, got %d" % (what, name, B, x.shape[0]))
        return x
    if x.is_floating_point() or x.dtype == torch.bool or x.shape != (B,):
        raise ValueError("wavenet_speech_amd.%s: %s must be integers of shape (%d,), got %s %s" % (what, name, B, x.dtype, tuple(x.shape)))
    return x.detach().to(device=device, dtype=torch.int32).contiguous()


def scale_shift(x, B, device, what):
    """the [B, 2] float32 pair of an affine map per read, contiguous; None stays None"""
    if x is None:
        return None
    x = gpu_tensor(x, what, "scale_shift", (torch.float32,), ValueError, device)
    if tuple(x.shape) != (B, 2):
        raise ValueError("wavenet_speech_amd.%s: scale_shift must be [%d, 2], got %s" % (what, B, tuple(x.shape)))
    return x.contiguous()


def into_table(into, field, shape, device, what, dtype=torch.int64):
    """the table of `dtype` a call accumulates into: into.<field> itself (checked), or fresh zeros without one"""
    t = getattr(into, field) if into is not None else None
    if t is None:
        return torch.zeros(shape, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError("wavenet_speech_amd.%s: into.%s must be a contiguous %s tensor of shape %s on %s"
                         % (what, field, _names((dtype,)), shape, device))
    return t


MAX_AFFINE_COST = 1024        # of the doubled integer costs


def affine_costs(what, match, mismatch, gap_open, gap_extend):
    """the four costs of an affine-gap alignment (pairwise_align, demux) as the kernels' integers, in half units"""
    costs = []
    for name, v in (("match", match), ("mismatch", mismatch), ("gap_open", gap_open), ("gap_extend", gap_extend)):
        d = 2.0 * float(v)
        if d != int(d):
            raise ValueError("wavenet_speech_amd.%s: %s must be a multiple of 0.5, got %r" % (what, name, v))
        costs.append(int(d))
    if not (0 <= costs[3] <= costs[2] <= MAX_AFFINE_COST) or max(abs(costs[0]), abs(costs[1])) > MAX_AFFINE_COST:
        raise ValueError("wavenet_speech_amd.%s: need 0 <= gap_extend <= gap_open <= %g and |match|, |mismatch| <= %g, got %r"
                         % (what, MAX_AFFINE_COST / 2, MAX_AFFINE_COST / 2, (match, mismatch, gap_open, gap_extend)))
    return costs


def note_bad(bad, message, at_once=False):
    """look at the device flags of earlier calls, then hand this call's counter `bad` (int32 [1], or None) to the watch"""
    if bad is None:
        return
    _flags.WATCH.poll()
    _flags.WATCH.note(bad, message, at_once=at_once)
