"""
Host side of the hot path: torch.autograd.Function wrappers that drive libwavenet_amd.so through its
C ABI.  torch supplies device memory, the current HIP stream and autograd bookkeeping -- all arithmetic
(dilated convs, gate, 1x1 products, every gradient) runs in the HIP kernels.

There is no CPU path: CPU tensors raise.
"""
import collections
import ctypes
import functools
import os

import torch
from torch.autograd.function import once_differentiable

from . import _flags, _lib
from ._args import _alloc_bytes, _p, _stream  # noqa: F401  (tools and tests import them from here)
from .series import Lease, SeriesLayout, fresh_series, load_series, window

PARAMS_PER_BLOCK = 10  # order = _lib.BlockParams fields


class BlockSpec(object):
    """Static description of one residual block (modules/block.py:22-51 in the reference) as the C ABI sees it."""
    __slots__ = ("ci", "co", "ms", "k", "d", "causal")

    def __init__(self, ci, co, ms, k, d, causal):
        self.ci, self.co, self.ms, self.k, self.d, self.causal = int(ci), int(co), int(ms), int(k), int(d), bool(causal)

    def offsets(self):
        return _lib.tap_offsets(self.k, self.d, self.causal)

    def reach(self):
        return max(abs(o) for o in self.offsets())

    def key(self):
        return (self.ci, self.co, self.ms, self.k, self.d, self.causal)

    def param_shapes(self):
        """the ten parameter shapes in C-ABI order (1x1 convs as matrices)"""
        co, ci, k, ms = self.co, self.ci, self.k, self.ms
        return [(co, ci, k), (co,), (co, ci, k), (co,), (co, co), (co,), (ms, co), (ms,), (co, ci), (co,)]


def _on_device_of_first_tensor(fn):
    """Run an autograd.Function forward/backward with the CUDA/HIP device of its first tensor argument current, so
    that torch.cuda.current_stream() and the kernel launches of the C ABI target the device that owns the buffers."""
    @functools.wraps(fn)
    def wrapper(ctx, *args):
        dev = next((a.device for a in args if isinstance(a, torch.Tensor) and a.is_cuda), None)
        if dev is None:
            return fn(ctx, *args)
        with torch.cuda.device(dev):
            return fn(ctx, *args)
    return wrapper


def _require_device(t, what):
    if not t.is_cuda:
        raise RuntimeError("wavenet_speech_amd: %s is a CPU tensor; the HIP path needs ROCm device tensors "
                           "(there is no CPU fallback)" % what)
    if t.dtype != torch.float32:
        raise RuntimeError("wavenet_speech_amd: %s must be float32, got %s" % (what, t.dtype))


def _own(view):
    """Fresh contiguous copy of a window of a pooled buffer.  `.contiguous()` is NOT enough: when halo == 0, L is a
    multiple of 128 and C a multiple of 8 the padded layout is already dense and it would return the alias."""
    return view.clone(memory_format=torch.contiguous_format)


def _workspace(ws_bytes, device):
    return torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)


# what every step of one stack call shares
_Call = collections.namedtuple("_Call", "lib batch layout dev")


def _shape(spec, batch, layout):
    return _lib.BlockShape(batch, layout.length, spec.ci, spec.co, spec.ms, spec.k, spec.d, int(spec.causal),
                           layout.ld, layout.halo)


def _params_struct(tensors):
    return _lib.BlockParams(*[_p(t) for t in tensors])


def _prep_params(tensors, spec):
    """contiguous fp32 device copies (no-ops for ordinary nn.Parameters) + shape checks"""
    out = []
    for t, w in zip(tensors, spec.param_shapes()):
        _require_device(t, "parameter")
        if t.dim() == 3 and len(w) == 2:  # 1x1 Conv1d weights arrive as [Co][Ci][1]
            t = t[:, :, 0]
        if tuple(t.shape) != w:
            raise RuntimeError("wavenet_speech_amd: parameter shape %s, expected %s" % (tuple(t.shape), w))
        out.append(t.detach().contiguous())
    return out


def _pack_block(lib, shape, params, device):
    packed = _alloc_bytes(lib.wn_block_packed_bytes(ctypes.byref(shape)), "wn_block_packed_bytes", device)
    ps = _params_struct(params)
    _lib.check(lib.wn_block_pack(ctypes.byref(shape), ctypes.byref(ps), _p(packed), _stream()), "wn_block_pack")
    return packed


def _alloc_block_grads(spec, dr, device):
    """the ten gradient tensors of a block whose residual output has the gradient `dr`"""
    # the last block of a stack has no consumer of its residual output (dr is None): conv1x1_residual and
    # residual_proj then get NO gradient (None), exactly as autograd leaves them in the reference -- a zero tensor
    # would make weight-decay optimisers decay parameters the reference never touches
    unused = (4, 5, 8, 9) if dr is None else ()
    return [None if i in unused else torch.empty(s, dtype=torch.float32, device=device) for i, s in enumerate(spec.param_shapes())]


def _block_backward(c, shape, spec, packed, x, sg, z, dr, dskip, want_dx):
    """bwd-data + bwd-weights of one block; returns (dx lease or None, [10 gradient tensors])"""
    lib = c.lib
    da, dg = Lease(c.batch, spec.co, c.layout, c.dev), Lease(c.batch, spec.co, c.layout, c.dev)
    dx = Lease(c.batch, spec.ci, c.layout, c.dev) if want_dx else None
    _lib.check(lib.wn_block_backward_data(ctypes.byref(shape), _p(packed), _p(dr), _p(dskip), _p(z), _p(sg),
                                          _p(da), _p(dg), _p(dx), _stream()), "wn_block_backward_data")
    grads = _alloc_block_grads(spec, dr, c.dev)
    ws_bytes = lib.wn_block_wgrad_workspace_bytes(ctypes.byref(shape))
    ws = _workspace(ws_bytes, c.dev)
    gs = _params_struct(grads)
    _lib.check(lib.wn_block_backward_weights(ctypes.byref(shape), _p(x), _p(z), _p(da), _p(dg), _p(dr), _p(dskip),
                                             ctypes.byref(gs), _p(ws), ws_bytes, _stream()),
               "wn_block_backward_weights")
    return dx, grads


def _skipsum_shape(specs, idx, batch, layout):
    shape = _lib.SkipSumShape(batch, layout.length, specs[0].ms, len(idx), layout.ld, layout.halo)
    for i, l in enumerate(idx):
        shape.channels[i] = specs[l].co
    return shape


def _skipsum_groups(specs, zs, batch, layout):
    """(group number, its blocks, its SkipSumShape, its z pointers) of the long-K skips_sum products: <= MAX_STACK_GROUP blocks each"""
    G = _lib.MAX_STACK_GROUP
    for gi, g0 in enumerate(range(0, len(specs), G)):
        idx = range(g0, min(g0 + G, len(specs)))
        yield gi, idx, _skipsum_shape(specs, idx, batch, layout), (ctypes.c_void_p * len(idx))(*[zs[l].ptr for l in idx])


def _stack_skip_sum(c, specs, zs, skip_w, bias_total, S, packed_groups=None, leaky=None):
    """S = sum_l W_skip_l z_l + sum_l b_skip_l, in groups of <= MAX_STACK_GROUP blocks (one long-K GEMM each).
    packed_groups: the groups' packed weights when the stack's pack table has made them already.
    leaky: a slope -- S is then stored as leaky_relu(S) (one group only: the activation needs the complete sum)."""
    lib = c.lib
    assert leaky is None or len(specs) <= _lib.MAX_STACK_GROUP
    for gi, idx, shape, zptrs in _skipsum_groups(specs, zs, c.batch, c.layout):
        if packed_groups is not None:
            packed = packed_groups[gi]
        else:
            packed = _alloc_bytes(lib.wn_skipsum_packed_bytes(ctypes.byref(shape)), "wn_skipsum_packed_bytes", c.dev)
            wptrs = (ctypes.c_void_p * len(idx))(*[skip_w[l].data_ptr() for l in idx])
            _lib.check(lib.wn_skipsum_pack(ctypes.byref(shape), wptrs, _p(bias_total) if gi == 0 else None, _p(packed),
                                           _stream()), "wn_skipsum_pack")
        if leaky is not None:
            _lib.check(lib.wn_skipsum_forward_series(ctypes.byref(shape), _p(packed), zptrs, _p(S), ctypes.c_float(leaky), _stream()),
                       "wn_skipsum_forward_series")
        else:
            _lib.check(lib.wn_skipsum_forward(ctypes.byref(shape), _p(packed), zptrs, _p(S), 0 if gi == 0 else 1, _stream()),
                       "wn_skipsum_forward")


def _pack_conv(lib, shape, w, b, device):
    packed = _alloc_bytes(lib.wn_conv_packed_bytes(ctypes.byref(shape)), "wn_conv_packed_bytes", device,
                          -1 if shape.kernel_width <= _lib.MAX_TAPS else -2)
    _lib.check(lib.wn_conv_pack(ctypes.byref(shape), _p(w), _p(b), _p(packed), _stream()), "wn_conv_pack")
    return packed


def _conv_wgrad(lib, shape, xin, dy, wshape, has_bias, device):
    """(dW, db) of a conv whose input and output gradient are series already"""
    dw = torch.empty(wshape, dtype=torch.float32, device=device)
    db = torch.empty(wshape[0], dtype=torch.float32, device=device) if has_bias else None
    ws_bytes = lib.wn_conv_wgrad_workspace_bytes(ctypes.byref(shape))
    ws = _workspace(ws_bytes, device)
    _lib.check(lib.wn_conv_backward_weights(ctypes.byref(shape), _p(xin), _p(dy), _p(dw), _p(db), _p(ws), ws_bytes, _stream()),
               "wn_conv_backward_weights")
    return dw, db


class _PackTable(object):
    """What the pack-job tables of the fp32 path and of the half modes (functional_half.StackPackTable) share.  A table is built
    once per (shapes, layout, pointers) and holds pointers and shapes, never weight values.  Tensors computed anew every step
    (anything that is not an nn.Parameter: the folded bottleneck x skip products, the summed skip biases) are declared dynamic:
    the table holds their offsets inside their storages and each run supplies the storages' current addresses, so steady-state
    training never rebuilds it."""
    MAX_DYNAMIC = 3

    @staticmethod
    def dynamic_storages(tensors):
        """distinct storages of the tensors that are not nn.Parameters (recomputed every step), in first-seen order; None if too many"""
        seen = []
        for t in tensors:
            if t is not None and not isinstance(t, torch.nn.Parameter):
                st = t.untyped_storage()
                if all(st.data_ptr() != q.data_ptr() for q in seen):
                    seen.append(st)
        return seen if len(seen) <= _PackTable.MAX_DYNAMIC else None

    @staticmethod
    def relative(storages):
        """(the storages' sizes, rel): rel(t) is what a key holds of tensor t's address -- ("d", i, offset) inside dynamic storage i,
        so that the key outlives the storage moving, and the address itself anywhere else"""
        dyn = [(st.data_ptr(), st.nbytes()) for st in storages]

        def rel(t):
            if t is None:
                return None
            p = t.data_ptr()
            for i, (b, n) in enumerate(dyn):
                if b <= p < b + n:
                    return ("d", i, p - b)
            return p
        return tuple(n for _, n in dyn), rel

    @staticmethod
    def mem_ranges(storages):
        return (_lib.MemRange * max(1, len(storages)))(*[_lib.MemRange(st.data_ptr(), st.nbytes()) for st in storages])

    def bases(self, storages):
        return (ctypes.c_void_p * max(1, self.ndyn))(*[st.data_ptr() for st in storages])


class StackPackTable(_PackTable):
    """Device-resident table of every weight-pack job of an fp32 stack (wn_stack_pack_*): each block's four arrangements, in
    training the long-K skips_sum weights, and the convs around the stack that run in the same function.  ONE launch per step
    packs everything into one buffer."""

    @staticmethod
    def key_of(specs, B, layout, prepped, bias_total, convs, storages):
        sizes, rel = _PackTable.relative(storages)
        return ("f32", B, layout.key(), sizes, tuple(s.key() for s in specs),
                tuple(rel(t) for blk in prepped for t in blk), rel(bias_total),
                tuple((tuple(getattr(sh, f) for f, _ in sh._fields_), rel(w), rel(b)) for sh, w, b in convs))

    def __init__(self, lib, specs, B, layout, prepped, bias_total, convs, storages, device):
        n, nc = len(specs), len(convs)
        shapes = (_lib.BlockShape * n)(*[_shape(s, B, layout) for s in specs])
        params = (_lib.BlockParams * n)(*[_params_struct(blk) for blk in prepped])
        carr = (_lib.PackConv * max(1, nc))(*[_lib.PackConv(sh, _p(w), _p(b)) for sh, w, b in convs])
        nbytes = lib.wn_stack_pack_table_bytes(n, nc)
        host = ctypes.create_string_buffer(nbytes)
        offs = (ctypes.c_size_t * n)()
        soffs = (ctypes.c_size_t * ((n + _lib.MAX_STACK_GROUP - 1) // _lib.MAX_STACK_GROUP))()
        coffs = (ctypes.c_size_t * max(1, nc))()
        total, njobs, nblocks = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.wn_stack_pack_table_build(shapes, params, n, 1 if bias_total is not None else 0, _p(bias_total), carr, nc,
                                                 self.mem_ranges(storages), len(storages), host, nbytes, offs, soffs, coffs,
                                                 ctypes.byref(total), ctypes.byref(njobs), ctypes.byref(nblocks)),
                   "wn_stack_pack_table_build")
        self.table = torch.frombuffer(host, dtype=torch.uint8).to(device)      # the one host-to-device copy of the table's life
        self.njobs, self.launch_blocks, self.ndyn = njobs.value, nblocks.value, len(storages)
        self.block_offsets, self.conv_offsets = list(offs), list(coffs)[:nc]
        self.skipsum_offsets = list(soffs) if bias_total is not None else []
        self.total = total.value

    def run(self, lib, storages, device, out=None):
        """pack everything into a fresh buffer (or `out`); returns it (block l at data_ptr() + block_offsets[l])"""
        packed = torch.empty(self.total, dtype=torch.uint8, device=device) if out is None else out
        _lib.check(lib.wn_stack_pack_run(_p(self.table), self.njobs, self.launch_blocks, self.bases(storages), self.ndyn, _p(packed),
                                         _stream()), "wn_stack_pack_run")
        return packed


# ---- argument handling that the fp32 and the half stack functions share ---------------------------------------------------------
def _split_flat(flat, n, has_head, nfront):
    """(the blocks' tensors, head parameters or None, front parameters or None) of a stack function's `flat`: the front's `nfront`
    tensors are its LAST entries, the head's four (w1, b1, w2, b2) come right before them"""
    head_params = front_params = None
    if nfront:
        front_params = [None if t is None else t.detach().contiguous() for t in flat[-nfront:]]
        flat = flat[:-nfront]
    if has_head:
        head_params = [t.detach().contiguous() for t in flat[-4:]]
        flat = flat[:-4]
    assert len(flat) == n * PARAMS_PER_BLOCK
    return flat, head_params, front_params


def _pooled_length(L, pool, front, front_name):
    """length of the stack's input series when AvgPool1d(pool) is fused into its load (a tail shorter than the window is dropped)"""
    if pool > 1:
        if front is not None:
            raise RuntimeError("wavenet_speech_amd: pooling and a %s in front of one stack are not combined" % front_name)
        L = L // pool
        if L < 1:
            raise RuntimeError("wavenet_speech_amd: sequence shorter than the pooling window")
    return L


def _check_stack(specs, C0):
    """a stack's blocks take C0 input channels, chain, and share out_dim; returns out_dim"""
    if C0 != specs[0].ci:
        raise RuntimeError("wavenet_speech_amd: input has %d channels, first block expects %d" % (C0, specs[0].ci))
    for l in range(1, len(specs)):
        if specs[l].ci != specs[l - 1].co:   # the reference raises a conv1d shape error here
            raise RuntimeError("wavenet_speech_amd: block %d expects %d input channels but block %d produces %d"
                               % (l, specs[l].ci, l - 1, specs[l - 1].co))
    ms = specs[0].ms
    for spec in specs:
        if spec.ms != ms:
            raise RuntimeError("wavenet_speech_amd: all blocks of a stack must share out_dim")
    return ms


def _head_shapes(head_params, ms, batch, layout):
    """ConvShapes of the two 1x1 convs of an output block behind a stack of out_dim ms"""
    w1, _b1, w2, _b2 = head_params
    c1, c2 = w1.shape[0], w2.shape[0]
    if w1.shape[1] != ms or w2.shape[1] != c1 or w1.shape[2] != 1 or w2.shape[2] != 1:
        raise RuntimeError("wavenet_speech_amd: output block shapes %s, %s do not follow a stack of out_dim %d"
                           % (tuple(w1.shape), tuple(w2.shape), ms))
    return (_lib.ConvShape(batch, layout.length, ms, c1, 1, 1, 1, layout.ld, layout.halo),
            _lib.ConvShape(batch, layout.length, c1, c2, 1, 1, 1, layout.ld, layout.halo))


# ---- the steps of the fp32 stack function, in the order forward and backward run them ------------------------------------------------
def _pack_stack(c, pack_cache, frozen, specs, prepped, bias_total, convs, callers):
    """Every packed image of the call: (buffer that owns them or None, per block, per skips_sum group or None, per conv).
    All pack jobs (4 per block, in training the long-K skips_sum weights, the convs) come from ONE launch of a device-resident
    job table (StackPackTable); a frozen model keeps its packed weights instead; WN_PACK_TABLE=0 or parameters spread over too
    many non-Parameter storages fall back to the per-object entry points."""
    storages = None
    if pack_cache is not None and not frozen and os.environ.get("WN_PACK_TABLE", "1") != "0":
        # (whether a storage is dynamic is decided on the caller's tensors -- detach() makes a Parameter a plain tensor --,
        #  the addresses come from the prepared ones)
        storages = StackPackTable.dynamic_storages(callers + [bias_total])
    if storages is None:
        blocks = _pack_blocks(c, pack_cache, frozen, specs, lambda l, shape: _pack_block(c.lib, shape, prepped[l], c.dev))
        return None, blocks, None, [_pack_conv(c.lib, sh, w, b, c.dev) for sh, w, b in convs]
    key = StackPackTable.key_of(specs, c.batch, c.layout, prepped, bias_total, convs, storages)
    table = pack_cache.table(key, lambda: StackPackTable(c.lib, specs, c.batch, c.layout, prepped, bias_total, convs, storages, c.dev))
    packed_all = table.run(c.lib, storages, c.dev)
    base = packed_all.data_ptr()
    groups = [base + o for o in table.skipsum_offsets] if bias_total is not None else None
    return packed_all, [base + o for o in table.block_offsets], groups, [base + o for o in table.conv_offsets]


def _pack_blocks(c, pack_cache, frozen, specs, pack_one):
    """the per-object fallback, lazily: block l is packed (pack_one(l, its BlockShape)) when the block loop reaches it; a frozen
    model keeps the image"""
    for l, spec in enumerate(specs):
        packed = pack_cache.get(l, c.layout, c.batch) if frozen else None
        if packed is None:
            packed = pack_one(l, _shape(spec, c.batch, c.layout))
            if frozen:
                pack_cache.put(l, c.layout, c.batch, packed)
        yield packed


def _input_series(c, x, pool, entry):
    """The stack's input as a series: x itself, AvgPool1d(pool) of x (reference modules/classifier.py:53,102) fused into the load,
    or the output of the entry conv `entry` = (ConvShape, packed weights).  Returns (series, the entry conv's input series or None)."""
    B, Cx, Lx = x.shape
    if entry is not None:
        fshape, fpk = entry
        xin = Lease(B, Cx, c.layout, c.dev)
        load_series(xin.t, x.detach(), c.layout)
        cur = Lease(B, fshape.out_channels, c.layout, c.dev)
        _lib.check(c.lib.wn_conv_forward(ctypes.byref(fshape), _p(fpk), _p(xin), _p(cur), _stream()), "wn_conv_forward")
        return cur, xin
    cur = Lease(B, Cx, c.layout, c.dev)
    if pool > 1:
        _lib.check(c.lib.wn_series_load_pooled(_p(x.detach().contiguous()), _p(cur), B, Cx, Lx, int(pool), c.layout.ld,
                                               c.layout.halo, _stream()), "wn_series_load_pooled")
    else:
        load_series(cur.t, x.detach(), c.layout)
    return cur, None


def _forward_blocks(c, specs, blocks_packed, series, S, training):
    """the block loop over the input `series` (a one-element list, emptied here); returns what backward needs of every block,
    [(x, sg, z, packed, shape)] (empty unless training)"""
    cur = series.pop()
    saved = []
    zbuf = None
    for l, (spec, packed) in enumerate(zip(specs, blocks_packed)):
        shape = _shape(spec, c.batch, c.layout)
        r = Lease(c.batch, spec.co, c.layout, c.dev) if l + 1 < len(specs) else None  # the last residual output is never used
        if training:
            sg, z = (Lease(c.batch, spec.co, c.layout, c.dev) for _ in range(2))   # kept for backward; tanh = z / sg
        else:
            sg = None
            if zbuf is None or zbuf.channels != spec.co:
                zbuf = Lease(c.batch, spec.co, c.layout, c.dev)
            z = zbuf
        # training keeps every block's z, so skips_sum is formed afterwards by one long-K product over all
        # blocks (wn_skipsum_forward); inference accumulates per block and keeps a single z scratch buffer
        _lib.check(c.lib.wn_block_forward(ctypes.byref(shape), _p(packed), _p(cur), _p(r), None if training else _p(S),
                                          1, _p(sg), _p(z), _stream()), "wn_block_forward")
        if training:
            saved.append((cur, sg, z, packed, shape))
        cur = r
    return saved


def _head_backward(c, ctx, d_out):
    """Output block, backwards, in the series: d_out is the cotangent of ITS output; each LeakyReLU backward rides in the epilogue
    of the backward-data product above it (mask = the stored activation).  Returns (dS, [dw1, db1, dw2, db2])."""
    lib = c.lib
    (slope1, slope2), sh1, sh2, pk1, pk2, h0, h1, hshapes = ctx.head
    dY = Lease(c.batch, sh2.out_channels, c.layout, c.dev)
    load_series(dY.t, d_out, c.layout)
    dw2, db2 = _conv_wgrad(lib, sh2, h1, dY, hshapes[2], True, c.dev)
    dh1 = Lease(c.batch, sh1.out_channels, c.layout, c.dev)
    _lib.check(lib.wn_conv_backward_data_series(ctypes.byref(sh2), _p(pk2), _p(dY), _p(h1), ctypes.c_float(slope2), _p(dh1),
                                                _stream()), "wn_conv_backward_data_series")
    del dY
    dw1, db1 = _conv_wgrad(lib, sh1, h0, dh1, hshapes[0], True, c.dev)
    dS = Lease(c.batch, sh1.in_channels, c.layout, c.dev)
    _lib.check(lib.wn_conv_backward_data_series(ctypes.byref(sh1), _p(pk1), _p(dh1), _p(h0), ctypes.c_float(slope1), _p(dS),
                                                _stream()), "wn_conv_backward_data_series")
    del dh1, h0, h1
    ctx.head = None
    return dS, [dw1, db1, dw2, db2]


def _backward_chain(c, ctx, dS):
    """the blocks, top to bottom; returns (gradient series of the stack's input or None, the blocks' gradients, flat)"""
    dr = None
    grads_flat = [None] * (len(ctx.specs) * PARAMS_PER_BLOCK)
    for l in range(len(ctx.specs) - 1, -1, -1):
        x, sg, z, packed, shape = ctx.saved[l]
        want_dx = l > 0 or ctx.front is not None or ctx.needs_input_grad[0]
        dr, grads = _block_backward(c, shape, ctx.specs[l], packed, x, sg, z, dr, dS, want_dx)
        grads_flat[l * PARAMS_PER_BLOCK:(l + 1) * PARAMS_PER_BLOCK] = grads
        ctx.saved[l] = None  # release this block's activations to the pool
    return dr, grads_flat


def _entry_backward(c, ctx, dr):
    """the conv in front, backwards: dr is the gradient of its output, a series already.  Returns (gradient series of ITS input
    or dr, [dw, db])"""
    xin, fpk, fshape, wshape, has_bias = ctx.front
    dw, db = _conv_wgrad(c.lib, fshape, xin, dr, wshape, has_bias, c.dev)
    if ctx.needs_input_grad[0]:
        dxin = Lease(c.batch, fshape.in_channels, c.layout, c.dev)
        _lib.check(c.lib.wn_conv_backward_data(ctypes.byref(fshape), _p(fpk), _p(dr), _p(dxin), _stream()),
                   "wn_conv_backward_data")
        dr = dxin
    ctx.front = None
    return dr, [dw, db]


class _ResidualStackFn(torch.autograd.Function):
    """The per-layer loop of WaveNet / RawCTCNet / WaveNetClassifier
    (modules/wavenet.py:98-100, raw_ctcnet.py:138-145, classifier.py:105-112):
        for l: out, skip = block_l(out); skips_sum = skips_sum + bottleneck_l(skip)
    with the bottleneck folded into the skip projection by the caller.  Returns skips_sum [B, Ms, L] -- or, with `head`,
    the output of the model's output block, which then runs here in the series layout; with `front` the entry conv in front of
    the stack runs here too and x is ITS input."""

    @staticmethod
    @_on_device_of_first_tensor
    def forward(ctx, x, specs, grad_enabled, pack_cache, pool, head, front, *flat):
        """arguments as residual_stack's; head = its slopes, front = its geometry, their parameters at the end of `flat` (_split_flat);
        pool > 1: AvgPool1d(pool) of x (reference modules/classifier.py:53,102) fused into the load of the stack's input series"""
        lib = _lib.load()
        _require_device(x, "input")
        n = len(specs)
        callers = list(flat)
        flat, head_params, front_params = _split_flat(flat, n, head is not None, 0 if front is None else 2)
        B, C0, L = x.shape
        ctx.pool, ctx.in_length = int(pool), L
        L = _pooled_length(L, pool, front, "conv")
        reach = max(s.reach() for s in specs)
        if front is not None:
            fk, fd, fcausal = front
            fw, fb = front_params
            _require_device(fw, "weight")
            if fw.dim() != 3 or fw.shape[1] != C0 or fw.shape[2] != fk:
                raise RuntimeError("wavenet_speech_amd: input has %d channels, conv expects %s" % (C0, tuple(fw.shape)))
            Cin, C0 = C0, fw.shape[0]
            reach = max(reach, max(abs(o) for o in _lib.tap_offsets(fk, fd, fcausal)))
        ms = _check_stack(specs, C0)
        layout = SeriesLayout(L, reach)
        c = _Call(lib, B, layout, x.device)
        # needs_input_grad reflects requires_grad of the arguments whatever the grad mode, and grad mode is always off
        # inside Function.forward: the caller captures torch.is_grad_enabled() and hands it in
        training = bool(grad_enabled) and any(ctx.needs_input_grad)
        ctx.training = training
        prepped = [_prep_params(flat[l * PARAMS_PER_BLOCK:(l + 1) * PARAMS_PER_BLOCK], spec) for l, spec in enumerate(specs)]
        bias_total = torch.stack([p[7] for p in prepped]).sum(0).contiguous() if training else None
        # the convs around the stack that run in this function: (shape, weight, bias)
        convs = []
        if front is not None:
            convs.append((_lib.ConvShape(B, L, Cin, C0, fk, fd, int(bool(fcausal)), layout.ld, layout.halo), fw, fb))
        if head is not None:
            sh1, sh2 = _head_shapes(head_params, ms, B, layout)
            convs += [(sh1, head_params[0], head_params[1]), (sh2, head_params[2], head_params[3])]
        frozen = pack_cache is not None and pack_cache.frozen and not grad_enabled
        # every packed image of the call lives in ctx.packed_all until backward has run
        ctx.packed_all, blocks_packed, groups, conv_packed = _pack_stack(c, pack_cache, frozen, specs, prepped, bias_total, convs, callers)

        cur, xin = _input_series(c, x, pool, (convs[0][0], conv_packed[0]) if front is not None else None)
        ctx.front = (xin, conv_packed[0], convs[0][0], tuple(fw.shape), fb is not None) if front is not None and training else None
        # with a head in training the long-K product writes leaky(S) straight into the head's input series: no dense S at all
        series_head = head is not None and training and n <= _lib.MAX_STACK_GROUP
        S = None if series_head else fresh_series(B, ms, layout, x.device)
        series = [cur]       # handed over: the loop drops each block's input once nothing needs it any more
        del cur
        saved = _forward_blocks(c, specs, blocks_packed, series, S, training)
        h0 = Lease(B, ms, layout, x.device) if head is not None else None
        if training:
            _stack_skip_sum(c, specs, [sv[2] for sv in saved], [p[6] for p in prepped], bias_total, h0 if series_head else S,
                            packed_groups=groups, leaky=head[0] if series_head else None)
        ctx.specs, ctx.saved, ctx.layout, ctx.batch = specs, saved, layout, B
        ctx.param_shapes = [tuple(t.shape) for t in flat]
        ctx.head = None
        if head is None:
            # hand autograd a tensor of its own: views of internal buffers must never escape a custom Function
            return window(S, ms, layout).clone(memory_format=torch.contiguous_format)
        # ---- output block in the series layout: leaky(S) -> conv1 -> leaky -> conv2 ------------------------------------------
        if not series_head:
            # (inference, or more blocks than one long-K group: S is a complete series here)
            window(h0.t, ms, layout).copy_(torch.nn.functional.leaky_relu(window(S, ms, layout), head[0]))
        pk1, pk2 = conv_packed[-2], conv_packed[-1]
        h1 = Lease(B, sh1.out_channels, layout, x.device)
        _lib.check(lib.wn_conv_forward_series(ctypes.byref(sh1), _p(pk1), _p(h0), _p(h1), ctypes.c_float(head[1]), _stream()),
                   "wn_conv_forward_series")
        y = Lease(B, sh2.out_channels, layout, x.device)
        _lib.check(lib.wn_conv_forward(ctypes.byref(sh2), _p(pk2), _p(h1), _p(y), _stream()), "wn_conv_forward")
        if training:
            ctx.head = (head, sh1, sh2, pk1, pk2, h0, h1, [tuple(t.shape) for t in head_params])
        return _own(y.view())

    @staticmethod
    @once_differentiable
    @_on_device_of_first_tensor
    def backward(ctx, d_out):
        c = _Call(_lib.load(), ctx.batch, ctx.layout, d_out.device)
        head_grads, front_grads = [], []
        if ctx.head is None:
            dS = Lease(c.batch, ctx.specs[0].ms, c.layout, c.dev)
            load_series(dS.t, d_out, c.layout)
        else:
            dS, head_grads = _head_backward(c, ctx, d_out)
        dr, grads_flat = _backward_chain(c, ctx, dS)
        if ctx.front is not None:
            dr, front_grads = _entry_backward(c, ctx, dr)
        dx0 = _own(dr.view()) if ctx.needs_input_grad[0] else None
        if dx0 is not None and ctx.pool > 1:
            dx0 = _unpool(c.lib, dx0, ctx.in_length, ctx.pool)
        ctx.packed_all = None
        # 1x1 Conv1d weights come in as [Co][Ci][1]; hand each gradient back in its parameter's own shape
        grads_flat = [None if g is None else g.view(shp) for g, shp in zip(grads_flat, ctx.param_shapes)]
        return (dx0, None, None, None, None, None, None) + tuple(grads_flat) + tuple(head_grads) + tuple(front_grads)


def _unpool(lib, dpooled, length, pool):
    """backward of the pooled load: each pooled gradient / pool, broadcast to its pool columns (0 for a dropped tail)"""
    B, C, _ = dpooled.shape
    dx = torch.empty(B, C, length, dtype=torch.float32, device=dpooled.device)
    _lib.check(lib.wn_pool_backward(_p(dpooled.contiguous()), _p(dx), B, C, length, int(pool), _stream()), "wn_pool_backward")
    return dx


class PackCache(object):
    """Per-stack packing state.

    * `tables` (always on): device-resident pack-job tables, of the fp32 path (StackPackTable) and of the half-precision modes
      (functional_half.StackPackTable) alike -- they hold pointers and shapes, never weight VALUES, so every forward still packs
      the current weights (one launch).
    * `packed` (only when `frozen`, see modules.block.freeze_for_inference): the packed weights themselves, kept across
      no_grad forwards.  The owner calls `validate(params)` before each use; an in-place update through the autograd-visible
      API (optimizer step, load_state_dict, p.mul_()) bumps a parameter's `_version` and empties the cache, so does a
      parameter moving to other storage.  Updates through `p.data` (p.data.mul_(2)) are invisible to torch's version counter:
      that is why keeping packed weights is opt-in."""

    MAX_TABLES = 8
    MAX_SHAPES = 4        # distinct (series layout, batch) shapes whose packed weights are kept (variable-length inference would
                          # otherwise keep one packed copy of every block per utterance length: ADVICE r02)

    def __init__(self):
        self.key = None
        self.packed = {}
        self._shapes = []          # the shapes in `packed`, least recently used first
        self.hits = 0
        self.tables = {}           # device-resident pack-job tables, by their key (False: the layout is not covered by a table)
        self.frozen = False        # keep packed weights / folded bottlenecks across no_grad forwards (opt-in)

    def table(self, key, build):
        """The pack-job table under `key`, made by build() at its first use.  None where build() raised NotImplementedError (a
        layout that the table does not cover: remembered, so that it is not tried again every step).  A full cache starts over."""
        t = self.tables.get(key)
        if t is None:
            try:
                t = build()
            except NotImplementedError:
                t = False
            if len(self.tables) >= self.MAX_TABLES:
                self.tables.clear()
            self.tables[key] = t
        return t or None

    def validate(self, params, extra=()):
        key = tuple((id(p), p._version, p.data_ptr(), p.device) for p in params) + tuple(extra)
        if key != self.key:
            self.key = key
            self.packed = {}
            self._shapes = []

    def get(self, l, layout, batch):
        shape = (layout.key(), batch)
        t = self.packed.get((l,) + shape)
        if t is not None:
            self.hits += 1
            self._touch(shape)
        return t

    def put(self, l, layout, batch, t):
        shape = (layout.key(), batch)
        self._touch(shape)
        self.packed[(l,) + shape] = t
        return t

    def _touch(self, shape):
        order = self._shapes
        if shape in order:
            order.remove(shape)
        order.append(shape)
        while len(order) > self.MAX_SHAPES:
            old = order.pop(0)                       # least recently used shape: drop its packed weights
            for k in [k for k in self.packed if k[1:] == old]:
                del self.packed[k]


def residual_stack(x, specs, flat_params, precision="f32", pack_cache=None, head=None, front=None, pool=1):
    """skips_sum of a stack of residual blocks.  flat_params: 10 tensors per block in C-ABI order
    (w_tanh, b_tanh, w_sigmoid, b_sigmoid, w_res [Co,Co,1], b_res, w_skip [Ms,Co], b_skip, w_proj, b_proj).
    precision: "f32" (exact fp32 MFMA, default) or one of the half-precision MFMA modes of functional_half.
    head: None, or ((slope1, slope2), [w1, b1, w2, b2]) of an output block LeakyReLU, Conv1d 1x1, LeakyReLU, Conv1d 1x1 that is to
    run inside the same function, in the series layout: the result is then that block's output, not skips_sum.
    front ("f32"): None, or ((k, dilation, causal), [weight, bias or None]) of a dilated conv in front of the stack (WaveNet's
    entry conv): x is then that conv's input and its output goes to the first block as a series.  In the half modes `front` is
    the feature layer of functional_half.residual_stack."""
    if precision != "f32":
        from . import functional_half
        return functional_half.residual_stack(x, specs, flat_params, precision, pack_cache, head, front, pool)
    flat = list(flat_params)
    hs = fs = None
    if head is not None:
        hs = (float(head[0][0]), float(head[0][1]))
        flat += list(head[1])
    if front is not None:
        fs = (int(front[0][0]), int(front[0][1]), bool(front[0][2]))
        flat += list(front[1])
    return _ResidualStackFn.apply(x, tuple(specs), torch.is_grad_enabled(), pack_cache, int(pool), hs, fs, *flat)


class _ResidualBlockFn(torch.autograd.Function):
    """Stand-alone ResidualBlock.forward (modules/block.py:54-82): returns (residual_out, skip_out)."""

    @staticmethod
    @_on_device_of_first_tensor
    def forward(ctx, x, spec, grad_enabled, *params):
        lib = _lib.load()
        _require_device(x, "input")
        B, C0, L = x.shape
        if C0 != spec.ci:
            raise RuntimeError("wavenet_speech_amd: input has %d channels, block expects %d" % (C0, spec.ci))
        dev = x.device
        layout = SeriesLayout(L, spec.reach())
        shape = _shape(spec, B, layout)
        prm = _prep_params(params, spec)
        packed = _pack_block(lib, shape, prm, dev)
        xin = Lease(B, C0, layout, dev)
        load_series(xin.t, x.detach(), layout)
        r = Lease(B, spec.co, layout, dev)
        s = Lease(B, spec.ms, layout, dev)
        training = bool(grad_enabled) and any(ctx.needs_input_grad)
        sg = Lease(B, spec.co, layout, dev) if training else None
        z = Lease(B, spec.co, layout, dev)
        _lib.check(lib.wn_block_forward(ctypes.byref(shape), _p(packed), _p(xin), _p(r), _p(s), 0,
                                        _p(sg), _p(z), _stream()), "wn_block_forward")
        if training:
            ctx.saved = (xin, sg, z, packed, shape)
        ctx.spec, ctx.layout, ctx.batch = spec, layout, B
        ctx.param_shapes = [tuple(t.shape) for t in params]
        return _own(r.view()), _own(s.view())

    @staticmethod
    @once_differentiable
    @_on_device_of_first_tensor
    def backward(ctx, d_r, d_s):
        lib = _lib.load()
        spec, layout, B = ctx.spec, ctx.layout, ctx.batch
        dev = d_r.device
        x, sg, z, packed, shape = ctx.saved
        dr, ds = Lease(B, spec.co, layout, dev), Lease(B, spec.ms, layout, dev)
        load_series(dr.t, d_r, layout)
        load_series(ds.t, d_s, layout)
        dx, grads = _block_backward(_Call(lib, B, layout, dev), shape, spec, packed, x, sg, z, dr, ds, ctx.needs_input_grad[0])
        grads = [g.view(shp) for g, shp in zip(grads, ctx.param_shapes)]
        dx0 = _own(dx.view()) if dx is not None else None
        ctx.saved = None
        return (dx0, None, None) + tuple(grads)


def residual_block(x, spec, params):
    """(residual_out, skip_out) of one block; params in C-ABI order with w_res / w_skip as [Co,Co,1] Conv1d weights."""
    return _ResidualBlockFn.apply(x, spec, torch.is_grad_enabled(), *params)


class _DilatedConvFn(torch.autograd.Function):
    """CausalConv1d / NonCausalConv1d forward (modules/conv_ops.py:39-44, 73-79); k=1 gives a 1x1 Conv1d."""

    @staticmethod
    @_on_device_of_first_tensor
    def forward(ctx, x, weight, bias, dilation, causal, grad_enabled):
        lib = _lib.load()
        _require_device(x, "input")
        _require_device(weight, "weight")
        B, Ci, L = x.shape
        Co, Ci_w, k = weight.shape
        if Ci_w != Ci:
            raise RuntimeError("wavenet_speech_amd: input has %d channels, conv expects %d" % (Ci, Ci_w))
        dev = x.device
        reach = max(abs(o) for o in _lib.tap_offsets(k, dilation, causal))
        layout = SeriesLayout(L, reach)
        shape = _lib.ConvShape(B, L, Ci, Co, k, int(dilation), int(bool(causal)), layout.ld, layout.halo)
        w = weight.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        packed = _pack_conv(lib, shape, w, b, dev)
        xin = Lease(B, Ci, layout, dev)
        load_series(xin.t, x.detach(), layout)
        y = Lease(B, Co, layout, dev)
        _lib.check(lib.wn_conv_forward(ctypes.byref(shape), _p(packed), _p(xin), _p(y), _stream()), "wn_conv_forward")
        if grad_enabled and any(ctx.needs_input_grad):
            ctx.saved = (xin, packed, shape)
        ctx.layout, ctx.dims, ctx.has_bias = layout, (B, Ci, Co, k), bias is not None
        return _own(y.view())

    @staticmethod
    @once_differentiable
    @_on_device_of_first_tensor
    def backward(ctx, d_y):
        lib = _lib.load()
        xin, packed, shape = ctx.saved
        layout = ctx.layout
        B, Ci, Co, k = ctx.dims
        dev = d_y.device
        dy = Lease(B, Co, layout, dev)
        load_series(dy.t, d_y, layout)
        dx0 = None
        if ctx.needs_input_grad[0]:
            dx = Lease(B, Ci, layout, dev)
            _lib.check(lib.wn_conv_backward_data(ctypes.byref(shape), _p(packed), _p(dy), _p(dx), _stream()),
                       "wn_conv_backward_data")
            dx0 = _own(dx.view())
        dw, db = _conv_wgrad(lib, shape, xin, dy, (Co, Ci, k), ctx.has_bias, dev)
        ctx.saved = None
        return dx0, dw, db, None, None, None


def dilated_conv(x, weight, bias, dilation=1, causal=True, precision="f32"):
    if precision != "f32":
        from . import functional_half
        return functional_half.conv(x, weight, bias, dilation, causal, precision)
    return _DilatedConvFn.apply(x, weight, bias, int(dilation), bool(causal), torch.is_grad_enabled())


class _SequenceNLLFn(torch.autograd.Function):
    """sum_t mean_b CE(logits[:, :, t], target[:, t])  (Loss.py:38-43) as one fused HIP pass each way."""

    @staticmethod
    @_on_device_of_first_tensor
    def forward(ctx, logits, target, grad_enabled=True):
        lib = _lib.load()
        _require_device(logits, "logits")
        if target.dtype != torch.int64 or not target.is_cuda:
            raise RuntimeError("wavenet_speech_amd: target must be an int64 device tensor")
        B, C, L = logits.shape
        x = logits.detach().contiguous()
        tg = target.contiguous()
        lse = torch.empty(2, B, L, dtype=torch.float32, device=x.device)   # (max, log sum exp(. - max)): csrc/wn_nll.hip
        partial = torch.empty(lib.wn_nll_partials(B, L), dtype=torch.float32, device=x.device)
        bad = torch.zeros(1, dtype=torch.int32, device=x.device)
        _lib.check(lib.wn_nll_forward(_p(x), _p(tg), _p(lse), _p(partial), _p(bad), B, C, L, _stream()), "wn_nll_forward")
        # the kernel never indexes the logits with an out-of-range label (it counts it and poisons the loss with NaN); the count
        # becomes an exception without stalling the stream in training calls (see _flags.py; WN_NLL_CHECK=0 skips it)
        if os.environ.get("WN_NLL_CHECK", "1") != "0":
            _flags.WATCH.poll()
            _flags.WATCH.note(bad, lambda n, C=C: "wavenet_speech_amd: sequence_nll got %d target(s) outside [0, %d)" % (n, C),
                              at_once=not (grad_enabled and ctx.needs_input_grad[0]))
        ctx.save_for_backward(x, tg, lse)
        return partial.sum() / B

    @staticmethod
    @once_differentiable
    @_on_device_of_first_tensor
    def backward(ctx, g):
        lib = _lib.load()
        x, tg, lse = ctx.saved_tensors
        B, C, L = x.shape
        gscale = (g / B).to(torch.float32).reshape(1).contiguous()
        dx = torch.empty_like(x)
        _lib.check(lib.wn_nll_backward(_p(x), _p(tg), _p(lse), _p(gscale), _p(dx), B, C, L, _stream()), "wn_nll_backward")
        return dx, None, None


def sequence_nll(logits, target):
    return _SequenceNLLFn.apply(logits, target, torch.is_grad_enabled())


class _EmbedConvFn(torch.autograd.Function):
    """CausalConv1d(d=1) applied to one_hot(levels) (modules/wavenet.py:54,93 + modules/fns.py:6-15) as a gather of weight
    columns: the [B, classes, L] one-hot is never built."""

    @staticmethod
    @_on_device_of_first_tensor
    def forward(ctx, weight, bias, levels, grad_enabled=True):
        lib = _lib.load()
        _require_device(weight, "weight")
        if levels.dtype != torch.int64 or not levels.is_cuda or levels.dim() != 2:
            raise RuntimeError("wavenet_speech_amd: levels must be an int64 device tensor [B, L]")
        Co, classes, k = weight.shape
        B, L = levels.shape
        q = levels.contiguous()
        w = weight.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        y = torch.empty(B, Co, L, dtype=torch.float32, device=weight.device)
        bad = torch.zeros(1, dtype=torch.int32, device=weight.device)
        _lib.check(lib.wn_embed_forward(_p(q), _p(w), _p(b), _p(y), B, L, classes, Co, k, _p(bad), _stream()), "wn_embed_forward")
        if os.environ.get("WN_NLL_CHECK", "1") != "0":
            _flags.WATCH.poll()
            _flags.WATCH.note(bad, lambda n, classes=classes: "wavenet_speech_amd: %d thread(s) saw a level outside [0, %d)" % (n, classes),
                              at_once=not (grad_enabled and any(ctx.needs_input_grad)))
        ctx.save_for_backward(q)
        ctx.dims, ctx.has_bias = (B, L, classes, Co, k), bias is not None
        return y

    @staticmethod
    @once_differentiable
    @_on_device_of_first_tensor
    def backward(ctx, d_y):
        lib = _lib.load()
        (q,) = ctx.saved_tensors
        B, L, classes, Co, k = ctx.dims
        dev = d_y.device
        dy = d_y.contiguous()
        # the exact-fp32 weight-gradient GEMM (wgrad_kernel, fixed summation order) against a one-hot that exists only inside this
        # call: backward DOES materialise a one-hot (279 MB at 16 x 256 x 16000, from the lease pool); the forward pass and the
        # saved state never hold one.  (A gather-form kernel without it was 3.5x slower and was removed: csrc/wn_embed.hip.)
        layout = SeriesLayout(L, k - 1)
        shape = _lib.ConvShape(B, L, classes, Co, k, 1, 1, layout.ld, layout.halo)
        xin = Lease(B, classes, layout, dev)
        # a level outside [0, classes) was counted by the forward kernel (and raises, one call late in training calls): here it must
        # not become an out-of-bounds scatter (ROCm builds compile the index assert out) -- it contributes nothing, like in the kernels
        ok = (q >= 0) & (q < classes)
        window(xin.t, classes, layout).zero_().scatter_(1, q.clamp(0, classes - 1).unsqueeze(1), ok.unsqueeze(1).to(torch.float32))
        dyl = Lease(B, Co, layout, dev)
        load_series(dyl.t, dy, layout)
        dw, db = _conv_wgrad(lib, shape, xin, dyl, (Co, classes, k), ctx.has_bias, dev)
        return dw, db, None, None


def embed_conv(levels, weight, bias):
    """entry_conv1d(one_hot(levels)) without the one-hot: levels [B, L] int64 -> [B, Co, L]"""
    return _EmbedConvFn.apply(weight, bias, levels, torch.is_grad_enabled())


# ------------------------------------------------------------------------------------------------------------------
# measurement hooks
# ------------------------------------------------------------------------------------------------------------------
def profile_enable(on=True):
    lib = _lib.load()
    _lib.check(lib.wn_prof_enable(1 if on else 0), "wn_prof_enable")


def profile_reset():
    _lib.check(_lib.load().wn_prof_reset(), "wn_prof_reset")


def profile_read():
    return _lib.profile_read()
