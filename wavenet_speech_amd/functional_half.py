"""
Host side of the half-precision-MFMA modes of the residual stack ("f16x3", "f16", "bf16"): the same
torch.autograd.Function shape as functional._ResidualStackFn, driving the wn_h* entry points of the C ABI.

    f16x3  operands split into two fp16 planes, three MFMAs per product, fp32 accumulate: 22-bit operands, within 1e-4 of the fp32 path on conditioned models
           (same 1e-4 parity bar as the fp32 path) at 3/16 of the fp32 MFMA cost
    f16 / bf16   plain half storage + MFMA, fp32 accumulate (BASELINE configs[4] / configs[1]); their error is the
           storage format's (measured in tests/test_gpu_half.py), far from 1e-4 through 30 blocks

Activations live in the "half series" layout of include/wavenet_amd.h; torch supplies device memory (series.Lease with a
half dtype), the stream and autograd bookkeeping.  There is no CPU path.
"""
import collections
import ctypes
import os

import torch
from torch.autograd.function import once_differentiable

from . import _flags, _lib
from .functional import (PARAMS_PER_BLOCK, _alloc_block_grads, _alloc_bytes, _check_stack, _head_shapes, _on_device_of_first_tensor,
                         _p, _pack_blocks, _PackTable, _params_struct, _pooled_length, _prep_params, _require_device, _shape, _skipsum_groups,
                         _split_flat, _stream, _unpool, _workspace)
from .series import Lease

# The cotangent is scaled by a power of two so that max|d skips_sum| lands in [0.125, 0.25]: gradients may then grow by 2^18
# on their way back through the stack before fp16 overflows (the reference's random init grows ~sqrt(2) per block: 2^15 over
# 30 blocks).  The price is small because v_mfma_f32_32x32x16_f16 honours fp16 subnormals (tools/probes/mfma_f16_denorm.hip):
# below the normal range the lo plane just loses bits gradually -- an absolute floor of 3e-8, i.e. 2e-7 of a tensor whose
# largest element is 0.125.
GRAD_TARGET = 0.25


def _cp32(c):
    return (c + 31) // 32 * 32


class HalfLayout(object):
    """row geometry of the half series of one call (wn_hseries_layout)"""

    def __init__(self, length, max_abs_offset):
        self.length = int(length)
        self.ld, self.halo = _lib.hseries_layout(self.length, int(max_abs_offset))

    def key(self):
        return ("half", self.length, self.ld, self.halo)


class _Mode(object):
    def __init__(self, precision):
        self.name = precision
        self.code = _lib.PRECISIONS[precision]
        self.planes = 2 if precision == "f16x3" else 1
        self.dtype = torch.bfloat16 if precision == "bf16" else torch.float16


def _hlease(mode, batch, channels, layout, device):
    g = _cp32(channels) // 8
    return Lease(batch, channels, layout, device, dtype=mode.dtype, rows=mode.planes * g, pitch=layout.ld * 8)


_OVERFLOW_MSG = ("wavenet_speech_amd: fp16 overflow in the %s of the half-precision stack (a value beyond +-65504 after the "
                 "built-in 1/16 residual scaling); use precision='f32' or 'bf16' for this model")


def check_fp16_overflow():
    """wait for every outstanding device flag (see _flags.py) and raise if one is set"""
    _flags.check_device_flags()


_SCALE_ACC = {}      # per device: the absmax accumulator of wn_grad_scale


def _grad_scale(cotangent, mode):
    """(scale, 1 / scale) device scalars of a backward call: the dynamic power of two that puts max|cotangent| at GRAD_TARGET,
    computed on the device (no host sync).  bf16 has fp32's exponent range: its gradients need no scaling (None, None)."""
    if mode.dtype == torch.bfloat16:
        return None, None
    lib = _lib.load()
    dev = cotangent.device
    acc = _SCALE_ACC.get(dev)
    if acc is None:
        acc = _SCALE_ACC[dev] = torch.zeros(1, dtype=torch.int32, device=dev)   # (every call leaves it zero again)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    c = cotangent.contiguous()
    if c.data_ptr() % 16:
        c = c.clone()                     # (a view into the middle of a buffer: the kernel reads 16-byte vectors)
    _lib.check(lib.wn_grad_scale(_p(c), c.numel(), ctypes.c_float(GRAD_TARGET), _p(out), _p(acc), _stream()), "wn_grad_scale")
    return out[0:1], out[1:2]


# what every step of one call shares: _Call's fields, the arithmetic mode, the fp16 overflow flag (None in bf16), the residual scale
_HCall = collections.namedtuple("_HCall", "lib batch layout dev mode flag rs")


def _hcall(lib, batch, layout, dev, mode):
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if mode.dtype == torch.float16 else None
    return _HCall(lib, batch, layout, dev, mode, flag, float(lib.wn_hseries_residual_scale()))


def _lease(c, channels):
    return _hlease(c.mode, c.batch, channels, c.layout, c.dev)


def _load(lib, mode, dense, lease, layout, scale, dyn, flag):
    B, C, L = dense.shape
    _lib.check(lib.wn_hseries_load(mode.code, _p(dense), _p(lease), B, C, L, layout.ld, layout.halo, ctypes.c_float(scale),
                                   _p(dyn), _p(flag), _stream()), "wn_hseries_load")


def _pack_hconv(c, shape, w, b):
    packed = _alloc_bytes(c.lib.wn_hconv_packed_bytes(ctypes.byref(shape), c.mode.code), "wn_hconv_packed_bytes", c.dev,
                          -1 if shape.kernel_width <= _lib.MAX_TAPS else -2)
    _lib.check(c.lib.wn_hconv_pack(ctypes.byref(shape), c.mode.code, _p(w), _p(b), ctypes.c_float(c.rs), _p(packed), _stream()),
               "wn_hconv_pack")
    return packed


def _hconv_wgrad(c, shape, xin, dy, wshape, has_bias, dyn_inv):
    """(dW, db) of a half conv whose input and output gradient are series already"""
    dw = torch.empty(wshape, dtype=torch.float32, device=c.dev)
    db = torch.empty(wshape[0], dtype=torch.float32, device=c.dev) if has_bias else None
    ws_bytes = c.lib.wn_hconv_wgrad_workspace_bytes(ctypes.byref(shape), c.mode.code)
    ws = _workspace(ws_bytes, c.dev)
    _lib.check(c.lib.wn_hconv_backward_weights(ctypes.byref(shape), c.mode.code, _p(xin), _p(dy), ctypes.c_float(c.rs), _p(dw), _p(db),
                                               _p(dyn_inv), _p(ws), ws_bytes, _stream()), "wn_hconv_backward_weights")
    return dw, db


def plan_switches():
    """the per-call switches that change the packed layout of a half block (plan_hblock in csrc/wn_half_api.hip reads them at every
    call): whatever holds offsets into packed weights, or the weights themselves, is keyed by their current values"""
    return (os.environ.get("WN_FUSED_FWD"), os.environ.get("WN_COL_BWD"))


class StackPackTable(_PackTable):
    """Device-resident table of every weight-pack job of a half-mode stack (wn_hstack_pack_*): ONE launch per training step packs
    all blocks and the long-K skips_sum weights."""

    @staticmethod
    def key_of(specs, mode, B, layout, prepped, storages, skipsum):
        sizes, rel = _PackTable.relative(storages)
        return (mode.name, B, layout.key(), bool(skipsum), sizes, tuple(s.key() for s in specs),
                tuple(rel(t) for blk in prepped for t in blk)) + plan_switches()

    def __init__(self, lib, specs, mode, B, layout, prepped, storages, skipsum, device):
        n = len(specs)
        shapes = (_lib.BlockShape * n)(*[_shape(s, B, layout) for s in specs])
        params = (_lib.BlockParams * n)(*[_params_struct(blk) for blk in prepped])
        nbytes = lib.wn_hstack_pack_table_bytes(n)
        host = ctypes.create_string_buffer(nbytes)
        offs = (ctypes.c_size_t * n)()
        soffs = (ctypes.c_size_t * ((n + _lib.MAX_STACK_GROUP - 1) // _lib.MAX_STACK_GROUP))()
        total, njobs, nblocks = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
        rc = lib.wn_hstack_pack_table_build(shapes, params, n, mode.code, 1 if skipsum else 0, self.mem_ranges(storages), len(storages),
                                            host, nbytes, offs, soffs, ctypes.byref(total), ctypes.byref(njobs), ctypes.byref(nblocks))
        if rc == -2:
            raise NotImplementedError("layout not covered by the pack-job table")   # WN_ERR_UNSUPPORTED: per-block packing instead
        _lib.check(rc, "wn_hstack_pack_table_build")
        self.table = torch.frombuffer(host, dtype=torch.uint8).to(device)       # the one host-to-device copy of the table's life
        self.nblk, self.njobs, self.launch_blocks, self.ndyn = n, njobs.value, nblocks.value, len(storages)
        self.block_offsets = list(offs)
        self.skipsum_offsets = list(soffs)
        self.total = total.value

    def run(self, lib, storages, device, flag=None):
        """pack everything into a fresh buffer; returns it (block l at data_ptr() + block_offsets[l])"""
        packed = torch.empty(self.total, dtype=torch.uint8, device=device)
        _lib.check(lib.wn_hstack_pack_run(_p(self.table), self.nblk, self.njobs, self.launch_blocks, self.bases(storages), self.ndyn,
                                          _p(packed), _p(flag), _stream()), "wn_hstack_pack_run")
        return packed


def wgrad_groups(lib, shapes, precision_code, cap=None):
    """The weight-gradient launches of a backward pass.  `shapes`: the BlockShape of every block in the order backward reaches
    them (top block first).  Returns a list of (grouped, positions): grouped=False is one block on wn_hblock_backward_weights,
    grouped=True is one wn_hblocks_backward_weights launch over the blocks at those positions of `shapes`.

    Each block brings its own limit (wn_hblocks_wgrad_group_max; `cap`, if given, lowers it -- WN_WGRAD_GROUP).  A block of limit
    1 (ordinary pairs: > 128 channels) runs alone.  The others join the open group while the group stays within every member's
    limit and the library still plans it (wn_hblocks_wgrad_workspace_bytes > 0: no more than kMaxPair pairs); a block that does
    not fit starts the next group.  A stack of equal blocks therefore forms groups of its limit from the top, as before."""
    out, cur, cur_max = [], [], 0

    def close():
        if cur:
            out.append((True, list(cur)))
            del cur[:]

    for i, s in enumerate(shapes):
        lim = lib.wn_hblocks_wgrad_group_max(ctypes.byref(s), precision_code)
        if lim <= 0:
            _lib.check(-1, "wn_hblocks_wgrad_group_max")
        if cap is not None:
            lim = max(1, min(lim, int(cap)))
        if lim == 1:
            close()
            out.append((False, [i]))
            continue
        if cur:
            m = len(cur) + 1
            arr = (_lib.BlockShape * m)(*[shapes[j] for j in cur + [i]])
            if m > min(cur_max, lim) or lib.wn_hblocks_wgrad_workspace_bytes(arr, m, precision_code) == 0:
                close()
        if not cur:
            cur_max = lim
        cur.append(i)
        cur_max = min(cur_max, lim)
        if len(cur) >= cur_max:
            close()
    close()
    return out


_WGRAD_GROUPS = {}   # wgrad_groups results by (precision, WN_WGRAD_GROUP, WN_HWGRAD_COMPOSITE, block shapes)


def _wgrad_plan(lib, mode, shapes):
    """(blocks whose weight gradients run in a group launch, blocks that close their group) for the BlockShapes of a stack.
    Small blocks (<= 128 channels) are two or three gradient tiles each -- their operands are kept and several blocks go into ONE
    split-K launch + ONE reduction (wn_hblocks_backward_weights); WN_WGRAD_GROUP=1 = per block.  The groups come from every
    block's own shape (wgrad_groups), in the order backward reaches the blocks: top first."""
    env_group = os.environ.get("WN_WGRAD_GROUP")
    order = list(range(len(shapes) - 1, -1, -1))
    top_down = [shapes[l] for l in order]
    gkey = (mode.code, env_group, os.environ.get("WN_HWGRAD_COMPOSITE"),
            tuple(tuple(getattr(s, f) for f, _ in s._fields_) for s in top_down))
    groups = _WGRAD_GROUPS.get(gkey)
    if groups is None:           # (the plan depends on the shapes only: planned once per stack geometry)
        groups = wgrad_groups(lib, top_down, mode.code, int(env_group) if env_group else None)
        if len(_WGRAD_GROUPS) >= 64:
            _WGRAD_GROUPS.clear()
        _WGRAD_GROUPS[gkey] = groups
    grouped, group_end = set(), set()
    for is_group, pos in groups:
        if is_group:
            grouped.update(order[p] for p in pos)
            group_end.add(order[pos[-1]])
    return grouped, group_end


def _flush_wgrad(c, pending, dS, dyn_inv):
    """ONE weight-gradient launch for the blocks in `pending` = [(shape, x, z, da, dg, dr, grads)], which it empties: their operands
    stay leased until here"""
    m = len(pending)
    if not pending:
        return
    shapes = (_lib.BlockShape * m)(*[e[0] for e in pending])
    arr = lambda i: (ctypes.c_void_p * m)(*[(e[i].ptr if e[i] is not None else None) for e in pending])
    dsk = (ctypes.c_void_p * m)(*[dS.ptr] * m)
    gs = (_lib.BlockParams * m)(*[_params_struct(e[6]) for e in pending])
    ws_bytes = c.lib.wn_hblocks_wgrad_workspace_bytes(shapes, m, c.mode.code)
    ws = _alloc_bytes(ws_bytes, "wn_hblocks_wgrad_workspace_bytes", c.dev)
    _lib.check(c.lib.wn_hblocks_backward_weights(shapes, m, c.mode.code, arr(1), arr(2), arr(3), arr(4), arr(5), dsk, gs,
                                                 _p(dyn_inv), _p(ws), ws_bytes, _stream()), "wn_hblocks_backward_weights")
    del pending[:]


# ---- the steps of the half stack function, in the order forward and backward run them -------------------------------------------------
def _input_series(c, x, pool, front, front_params):
    """The stack's input as a half series: x itself, AvgPool1d(pool) of x (reference modules/classifier.py:53,102) fused into the
    load, or the feature layer `front` = (slope0, slope1) of the raw signal x: leaky(conv k) (elementwise kernel) -> leaky(conv 1x1).
    Returns (series, what the feature layer's backward needs or None)."""
    lib, mode, lay = c.lib, c.mode, c.layout
    B, Cx, Lx = x.shape
    xd = x.detach().contiguous()
    if front is None:
        cur = _lease(c, Cx)
        if pool > 1:
            _lib.check(lib.wn_hseries_load_pooled(mode.code, _p(xd), _p(cur), B, Cx, Lx, int(pool), lay.ld, lay.halo,
                                                  ctypes.c_float(c.rs), None, _p(c.flag), _stream()), "wn_hseries_load_pooled")
        else:
            _load(c.lib, c.mode, xd, cur, c.layout, c.rs, None, c.flag)
        return cur, None
    fw0, fb0, fw1, fb1 = front_params
    F0, k0 = fw0.shape[0], fw0.shape[2]
    cur = _lease(c, fw1.shape[0])
    f1 = _lease(c, F0)
    _lib.check(lib.wn_hfeature_forward(mode.code, _p(xd), _p(fw0), _p(fb0), _p(f1), B, Lx, F0, k0, lay.ld, lay.halo,
                                       ctypes.c_float(c.rs), ctypes.c_float(front[0]), _p(c.flag), _stream()), "wn_hfeature_forward")
    fsh = _lib.ConvShape(B, lay.length, F0, fw1.shape[0], 1, 1, 1, lay.ld, lay.halo)
    fpk = _pack_hconv(c, fsh, fw1, fb1)
    _lib.check(lib.wn_hconv_forward_series(ctypes.byref(fsh), mode.code, _p(fpk), _p(f1), _p(cur), ctypes.c_float(c.rs),
                                           ctypes.c_float(front[1]), _p(c.flag), _stream()), "wn_hconv_forward_series")
    return cur, (front, xd, f1, fsh, fpk, Lx, [tuple(t.shape) for t in front_params])


def _pack_stack(c, pack_cache, frozen, specs, prepped, flat, training):
    """Every packed image of the stack: (buffer that owns them or None, per block, per skips_sum group or None).
    All pack jobs (5 per block + in training the long-K skips_sum weights) come from ONE launch of a device-resident job table
    (StackPackTable); a frozen model keeps its packed weights instead; WN_PACK_TABLE=0 or a layout that the table does not cover
    (e.g. skip biases that are not equally spaced) falls back to the per-block entry points."""
    table = None
    if pack_cache is not None and not frozen and os.environ.get("WN_PACK_TABLE", "1") != "0":
        storages = StackPackTable.dynamic_storages(flat)
        if storages is not None:
            key = StackPackTable.key_of(specs, c.mode, c.batch, c.layout, prepped, storages, training)
            table = pack_cache.table(key, lambda: StackPackTable(c.lib, specs, c.mode, c.batch, c.layout, prepped, storages, training,
                                                                 c.dev))
    if table is None:
        return None, _pack_blocks(c, pack_cache, frozen, specs, lambda l, shape: _pack_block(c, shape, prepped[l])), None
    packed_all = table.run(c.lib, storages, c.dev, c.flag)
    base = packed_all.data_ptr()
    return packed_all, [base + o for o in table.block_offsets], [base + o for o in table.skipsum_offsets]


def _pack_block(c, shape, params):
    packed = _alloc_bytes(c.lib.wn_hblock_packed_bytes(ctypes.byref(shape), c.mode.code), "wn_hblock_packed_bytes", c.dev)
    ps = _params_struct(params)
    _lib.check(c.lib.wn_hblock_pack_checked(ctypes.byref(shape), c.mode.code, ctypes.byref(ps), _p(packed), _p(c.flag), _stream()),
               "wn_hblock_pack_checked")
    return packed


def _forward_blocks(c, specs, blocks_packed, series, S, training):
    """the block loop over the input `series` (a one-element list, emptied here); returns what backward needs of every block,
    [(x, sg, z, packed, shape)] (empty unless training)"""
    lib, mode = c.lib, c.mode
    cur = series.pop()
    saved = []
    zbuf = None
    for l, (spec, packed) in enumerate(zip(specs, blocks_packed)):
        shape = _shape(spec, c.batch, c.layout)
        r = _lease(c, spec.co) if l + 1 < len(specs) else None
        if training:
            sg, z = (_lease(c, spec.co) for _ in range(2))   # kept for backward; tanh = z / sg
        elif lib.wn_hblock_forward_is_fused(ctypes.byref(shape), mode.code):
            sg = z = None                  # inference through the fused kernel: z stays on the chip
        else:
            sg = None
            if zbuf is None or zbuf.channels != spec.co:
                zbuf = _lease(c, spec.co)
            z = zbuf
        _lib.check(lib.wn_hblock_forward(ctypes.byref(shape), mode.code, _p(packed), _p(cur), _p(r),
                                         None if training else _p(S), 0 if l == 0 else 1, _p(sg), _p(z),
                                         _p(c.flag), _stream()), "wn_hblock_forward")
        if training:
            saved.append((cur, sg, z, packed, shape))
        cur = r
    return saved


def _skips_sum(c, specs, saved, prepped, groups, S):
    """The long-K skips_sum products of a training forward, their weights packed here where no table has done it: into the dense
    S, or, with S None (the head takes leaky(S) as a series: one group), not run -- the group's (shape, z pointers, packed
    weights) are returned for wn_hskipsum_forward_series."""
    lib, mode = c.lib, c.mode
    bias_total = torch.stack([p[7] for p in prepped]).sum(0).contiguous() if groups is None else None
    for gi, idx, shape, zptrs in _skipsum_groups(specs, [sv[2] for sv in saved], c.batch, c.layout):
        if groups is not None:
            packed = groups[gi]
        else:
            packed = _alloc_bytes(lib.wn_hskipsum_packed_bytes(ctypes.byref(shape), mode.code), "wn_hskipsum_packed_bytes", c.dev)
            wptrs = (ctypes.c_void_p * len(idx))(*[prepped[l][6].data_ptr() for l in idx])
            _lib.check(lib.wn_hskipsum_pack(ctypes.byref(shape), mode.code, wptrs, _p(bias_total) if gi == 0 else None,
                                            _p(packed), _stream()), "wn_hskipsum_pack")
        if S is not None:
            _lib.check(lib.wn_hskipsum_forward(ctypes.byref(shape), mode.code, _p(packed), zptrs, _p(S),
                                               0 if gi == 0 else 1, _stream()), "wn_hskipsum_forward")
    return shape, zptrs, packed


def _head_forward(c, head, head_params, S, series):
    """Output block in the series layout: leaky(S) -> conv1 -> leaky -> conv2 (dense fp32 out).  Its input is the dense S, or with
    `series` (_skips_sum's return) the long-K skips_sum product writes leaky(S) / 16 straight into the series: no dense fp32 S at all.
    Returns (y, what backward needs)."""
    lib, mode = c.lib, c.mode
    sh1, sh2 = _head_shapes(head_params, S.shape[1], c.batch, c.layout)
    pk = [_pack_hconv(c, sh1, head_params[0], head_params[1]), _pack_hconv(c, sh2, head_params[2], head_params[3])]
    h0 = _lease(c, sh1.in_channels)
    if series is not None:
        skshape, zptrs, skpacked = series
        _lib.check(lib.wn_hskipsum_forward_series(ctypes.byref(skshape), mode.code, _p(skpacked), zptrs, _p(h0),
                                                  ctypes.c_float(c.rs), ctypes.c_float(head[0]), _p(c.flag), _stream()),
                   "wn_hskipsum_forward_series")
    else:
        _load(c.lib, c.mode, torch.nn.functional.leaky_relu(S, head[0]), h0, c.layout, c.rs, None, c.flag)
    h1 = _lease(c, sh1.out_channels)
    _lib.check(lib.wn_hconv_forward_series(ctypes.byref(sh1), mode.code, _p(pk[0]), _p(h0), _p(h1), ctypes.c_float(c.rs),
                                           ctypes.c_float(head[1]), _p(c.flag), _stream()), "wn_hconv_forward_series")
    y = torch.empty(c.batch, sh2.out_channels, c.layout.length, dtype=torch.float32, device=c.dev)
    _lib.check(lib.wn_hconv_forward(ctypes.byref(sh2), mode.code, _p(pk[1]), _p(h1), _p(y), _stream()), "wn_hconv_forward")
    return y, (head, sh1, sh2, pk, h0, h1, [tuple(t.shape) for t in head_params])


def _head_backward(c, ctx, d_out, dyn, dyn_inv):
    """output block, backwards, in the series: d_out is the cotangent of its OUTPUT.  Returns (dS, [dw1, db1, dw2, db2])."""
    lib, mode = c.lib, c.mode
    (slope1, slope2), sh1, sh2, pk, h0, h1, hshapes = ctx.head
    dY = _lease(c, sh2.out_channels)
    _load(c.lib, c.mode, d_out, dY, c.layout, 1.0, dyn, c.flag)
    dh1 = _lease(c, sh1.out_channels)
    _lib.check(lib.wn_hconv_backward_data_series(ctypes.byref(sh2), mode.code, _p(pk[1]), _p(dY), _p(h1), ctypes.c_float(slope2),
                                                 _p(dh1), _p(c.flag), _stream()), "wn_hconv_backward_data_series")
    dS = _lease(c, sh1.in_channels)
    _lib.check(lib.wn_hconv_backward_data_series(ctypes.byref(sh1), mode.code, _p(pk[0]), _p(dh1), _p(h0), ctypes.c_float(slope1),
                                                 _p(dS), _p(c.flag), _stream()), "wn_hconv_backward_data_series")
    grads = _hconv_wgrad(c, sh1, h0, dh1, hshapes[0], True, dyn_inv) + _hconv_wgrad(c, sh2, h1, dY, hshapes[2], True, dyn_inv)
    ctx.head = None
    return dS, list(grads)


# The backward-data forms of a block.  dz is pointwise in time and its dr is the dx of the block above: where two consecutive blocks
# both take the column-owner kernels, dx of the upper and dz of the lower run as ONE launch (wn_hblock_backward_pair): the chain is
# then dz(top), [dx(l) + dz(l - 1)] ..., dx(bottom) -- n + 1 launches instead of 2 n.
BWD_TOP_PAIR = "dz of the top of a pair chain (no dx destination), then the pair launch"
BWD_PAIR = "pair launch: this block's dx + the dz of the block below"
BWD_INPUT = "bottom of a chain: the input gradient alone (series, masked by the feature layer's LeakyReLU, or dense)"
BWD_NOTHING = "bottom of a chain whose input needs no gradient: its dz (da, dg) is all that was needed"
BWD_MASKED = "dz + dx, the feature layer's LeakyReLU backward in the dx epilogue"
BWD_PLAIN = "dz + dx"


def backward_data_form(paired, have_dz, want_dx, want_dxd, masked):
    """The backward-data form of a block.  paired: it and the block below take the pair launch; have_dz: the pair launch above has
    produced its (da, dg) already; want_dx / want_dxd: its input gradient is wanted as a series / as a dense tensor;
    masked: its input is leaky(feature conv), whose backward rides in this block's dx epilogue."""
    if paired:
        return BWD_PAIR if have_dz else BWD_TOP_PAIR
    if have_dz:
        return BWD_INPUT if (want_dx or want_dxd) else BWD_NOTHING
    return BWD_MASKED if masked else BWD_PLAIN


def _backward_data(c, form, blk, below, dr, dS, gates, dx, dxd, dyn_inv, mask_slope):
    """launch `form` for the block blk = (x, sg, z, packed, shape) with gates = (da, dg); `below` is the block under it (pair forms).
    Returns the (da, dg) that a pair launch has produced for the block below, else None."""
    lib, code, flag = c.lib, c.mode.code, c.flag
    x, sg, z, packed, shape = blk
    da, dg = gates
    if form is BWD_TOP_PAIR or form is BWD_PLAIN:
        top = form is BWD_TOP_PAIR
        _lib.check(lib.wn_hblock_backward_data(ctypes.byref(shape), code, _p(packed), _p(dr), _p(dS), _p(z), _p(sg), _p(da), _p(dg),
                                               None if top else _p(dx), None if top else _p(dxd), _p(dyn_inv), _p(flag), _stream()),
                   "wn_hblock_backward_data")
    if form is BWD_TOP_PAIR or form is BWD_PAIR:
        _xl, sgl, zl, packedl, shapel = below
        dal, dgl = _lease(c, shapel.out_channels), _lease(c, shapel.out_channels)
        _lib.check(lib.wn_hblock_backward_pair(ctypes.byref(shape), _p(packed), ctypes.byref(shapel), _p(packedl), code,
                                               _p(dr), _p(da), _p(dg), _p(dS), _p(zl), _p(sgl), _p(dx), _p(dal), _p(dgl),
                                               _p(flag), _stream()), "wn_hblock_backward_pair")
        return dal, dgl
    if form is BWD_INPUT:
        masked = mask_slope is not None
        _lib.check(lib.wn_hblock_backward_input(ctypes.byref(shape), code, _p(packed), _p(dr), _p(da), _p(dg), _p(dx), _p(dxd),
                                                _p(dyn_inv), _p(x) if masked else None, ctypes.c_float(mask_slope if masked else 1.0),
                                                _p(flag), _stream()), "wn_hblock_backward_input")
    elif form is BWD_MASKED:
        # (x = the stored activation is the mask)
        _lib.check(lib.wn_hblock_backward_data_masked(ctypes.byref(shape), code, _p(packed), _p(dr), _p(dS), _p(z), _p(sg),
                                                      _p(da), _p(dg), _p(dx), _p(x), ctypes.c_float(mask_slope), _p(flag),
                                                      _stream()), "wn_hblock_backward_data_masked")
    return None


def _block_wgrad(c, blk, gates, dr, dS, grads, dyn_inv):
    """the weight gradients of one block on its own launch"""
    x, _sg, z, _packed, shape = blk
    ws_bytes = c.lib.wn_hblock_wgrad_workspace_bytes(ctypes.byref(shape), c.mode.code)
    ws = _workspace(ws_bytes, c.dev)
    gs = _params_struct(grads)
    _lib.check(c.lib.wn_hblock_backward_weights(ctypes.byref(shape), c.mode.code, _p(x), _p(z), _p(gates[0]), _p(gates[1]), _p(dr),
                                                _p(dS), ctypes.byref(gs), _p(dyn_inv), _p(ws), ws_bytes, _stream()),
               "wn_hblock_backward_weights")


def _backward_chain(c, ctx, dS, dyn_inv):
    """the blocks, top to bottom; returns (gradient series of the stack's input or None, its dense gradient or None, the blocks'
    gradients, flat)"""
    specs, saved = ctx.specs, ctx.saved
    grads_flat = [None] * (len(specs) * PARAMS_PER_BLOCK)
    grouped, group_end = _wgrad_plan(c.lib, c.mode, [sv[4] for sv in saved])
    pending = []          # blocks of a weight-gradient group whose launch is still to come
    dr = dx0 = None
    gates = None          # (da, dg) of the block about to be processed, if the pair launch above it has produced them
    for l in range(len(specs) - 1, -1, -1):
        spec, blk = specs[l], saved[l]
        have_dz = gates is not None
        da, dg = gates if have_dz else (_lease(c, spec.co), _lease(c, spec.co))
        dx = dxd = None
        if l > 0 or ctx.front is not None:
            dx = _lease(c, spec.ci)
        elif ctx.needs_input_grad[0]:
            dxd = dx0 = torch.empty(c.batch, spec.ci, c.layout.length, dtype=torch.float32, device=c.dev)
        paired = l > 0 and c.lib.wn_hblock_backward_pair_is_fused(ctypes.byref(blk[4]), ctypes.byref(saved[l - 1][4]), c.mode.code) == 1
        masked = l == 0 and ctx.front is not None
        form = backward_data_form(paired, have_dz, dx is not None, dxd is not None, masked)
        next_gates = _backward_data(c, form, blk, saved[l - 1] if paired else None, dr, dS, (da, dg), dx, dxd, dyn_inv,
                                    ctx.front[0][1] if masked else None)
        grads = _alloc_block_grads(spec, dr, c.dev)
        if l in grouped:
            pending.append((blk[4], blk[0], blk[2], da, dg, dr, grads))
            if l in group_end:
                _flush_wgrad(c, pending, dS, dyn_inv)
        else:
            _block_wgrad(c, blk, (da, dg), dr, dS, grads, dyn_inv)
        grads_flat[l * PARAMS_PER_BLOCK:(l + 1) * PARAMS_PER_BLOCK] = grads
        dr, gates = dx, next_gates
        saved[l] = None
    _flush_wgrad(c, pending, dS, dyn_inv)
    return dr, dx0, grads_flat


def _front_backward(c, ctx, dr, dyn_inv):
    """feature layer, backwards: dr is the (masked) gradient of the stack's input, in the series; returns [dw0, db0, dw1, db1]"""
    lib, mode, lay = c.lib, c.mode, c.layout
    (slope0, _slope1), xd, f1, fsh, fpk, L_in, fshapes = ctx.front
    F0, k0 = fsh.in_channels, fshapes[0][2]
    df1 = _lease(c, F0)
    _lib.check(lib.wn_hconv_backward_data_series(ctypes.byref(fsh), mode.code, _p(fpk), _p(dr), _p(f1), ctypes.c_float(slope0),
                                                 _p(df1), _p(c.flag), _stream()), "wn_hconv_backward_data_series")
    dw1, db1 = _hconv_wgrad(c, fsh, f1, dr, fshapes[2], True, dyn_inv)
    dw0 = torch.empty(fshapes[0], dtype=torch.float32, device=c.dev)
    db0 = torch.empty(fshapes[1], dtype=torch.float32, device=c.dev)
    ws_bytes = lib.wn_hfeature_wgrad_workspace_bytes(c.batch, L_in, F0, k0)
    ws0 = _workspace(ws_bytes, c.dev)
    _lib.check(lib.wn_hfeature_backward_weights(mode.code, _p(xd), _p(df1), ctypes.c_float(1.0), _p(dw0), _p(db0), c.batch, L_in, F0, k0,
                                                lay.ld, lay.halo, _p(dyn_inv), _p(ws0), ws_bytes, _stream()),
               "wn_hfeature_backward_weights")
    ctx.front = None
    return [dw0, db0, dw1, db1]


class _HalfStackFn(torch.autograd.Function):
    """skips_sum of a stack (modules/wavenet.py:98-100 with folded bottlenecks) on the half-precision MFMAs"""

    @staticmethod
    @_on_device_of_first_tensor
    def forward(ctx, x, specs, mode, grad_enabled, pack_cache, head, front, pool, *flat):
        """arguments as residual_stack's; head and front = their slopes, their parameters at the end of `flat` (_split_flat)"""
        lib = _lib.load()
        _require_device(x, "input")
        _flags.WATCH.poll()
        n = len(specs)
        flat, head_params, front_params = _split_flat(flat, n, head is not None, 0 if front is None else 4)
        B, C0, L = x.shape
        ctx.pool, ctx.in_length = int(pool), L
        L = _pooled_length(L, pool, front, "feature layer")
        if front is not None:
            fw0, fw1 = front_params[0], front_params[2]
            if C0 != 1 or fw0.shape[1] != 1 or fw1.shape[2] != 1 or fw1.shape[1] != fw0.shape[0]:
                raise RuntimeError("wavenet_speech_amd: feature layer shapes %s, %s do not fit a one-channel signal" %
                                   (tuple(fw0.shape), tuple(fw1.shape)))
            L = L + fw0.shape[2] - 1     # padding k - 1 on both sides lengthens the sequence (raw_ctcnet.py:57-61)
            C0 = fw1.shape[0]
        ms = _check_stack(specs, C0)
        training = bool(grad_enabled) and any(ctx.needs_input_grad)
        c = _hcall(lib, B, HalfLayout(L, max(s.reach() for s in specs)), x.device, mode)
        cur, front_saved = _input_series(c, x, pool, front, front_params)
        ctx.front = front_saved if training else None
        S = torch.empty(B, ms, L, dtype=torch.float32, device=x.device)
        prepped = [_prep_params(flat[l * PARAMS_PER_BLOCK:(l + 1) * PARAMS_PER_BLOCK], spec) for l, spec in enumerate(specs)]
        frozen = pack_cache is not None and pack_cache.frozen and not grad_enabled
        # the blocks' packed weights live in ctx.packed_all until backward has run
        ctx.packed_all, blocks_packed, groups = _pack_stack(c, pack_cache, frozen, specs, prepped, flat, training)
        series = [cur]       # handed over: the loop drops each block's input once nothing needs it any more
        del cur
        saved = _forward_blocks(c, specs, blocks_packed, series, S, training)
        series_head = head is not None and training and n <= _lib.MAX_STACK_GROUP
        ctx.skipsum_packed = sk = None
        if training:
            sk = _skips_sum(c, specs, saved, prepped, groups, None if series_head else S)
            if series_head:
                ctx.skipsum_packed = sk[2]
        ctx.head = None
        if head is not None:
            S, head_saved = _head_forward(c, head, head_params, S, sk if series_head else None)
            if training:
                ctx.head = head_saved
        _flags.WATCH.note(c.flag, _OVERFLOW_MSG % "forward pass", at_once=not training)
        ctx.specs, ctx.saved, ctx.layout, ctx.batch, ctx.mode = specs, saved, c.layout, B, mode
        ctx.param_shapes = [tuple(t.shape) for t in flat]
        return S

    @staticmethod
    @once_differentiable
    @_on_device_of_first_tensor
    def backward(ctx, d_skips):
        lib = _lib.load()
        _flags.WATCH.poll()
        d_skips = d_skips.contiguous()
        c = _hcall(lib, ctx.batch, ctx.layout, d_skips.device, ctx.mode)
        dyn, dyn_inv = _grad_scale(d_skips, c.mode)
        head_grads, front_grads = [], []
        if ctx.head is None:
            dS = _lease(c, ctx.specs[0].ms)
            _load(c.lib, c.mode, d_skips, dS, c.layout, 1.0, dyn, c.flag)
        else:
            dS, head_grads = _head_backward(c, ctx, d_skips, dyn, dyn_inv)
        dr, dx0, grads_flat = _backward_chain(c, ctx, dS, dyn_inv)
        if ctx.front is not None:
            front_grads = _front_backward(c, ctx, dr, dyn_inv)
        _flags.WATCH.note(c.flag, _OVERFLOW_MSG % "backward pass", at_once=False)
        grads_flat = [None if g is None else g.view(shp) for g, shp in zip(grads_flat, ctx.param_shapes)]
        if dx0 is not None and ctx.pool > 1:
            dx0 = _unpool(lib, dx0, ctx.in_length, ctx.pool)
        return (dx0, None, None, None, None, None, None, None) + tuple(grads_flat) + tuple(head_grads) + tuple(front_grads)


def residual_stack(x, specs, flat_params, precision, pack_cache=None, head=None, front=None, pool=1):
    """head: None, or ((slope1, slope2), [w1, b1, w2, b2]) of an output block LeakyReLU, Conv1d 1x1, LeakyReLU, Conv1d 1x1 that is
    to run inside the same function, in the half series: the result is then that block's output, not skips_sum.
    front: None, or ((slope0, slope1), [w0, b0, w1, b1]) of a feature layer Conv1d(1 -> F, k, padding k - 1), LeakyReLU, Conv1d 1x1,
    LeakyReLU in front of the stack: x is then the raw one-channel signal [B, 1, L]."""
    if precision not in ("f16x3", "f16", "bf16"):
        raise ValueError("unknown precision %r" % (precision,))
    flat = list(flat_params)
    hs = fs = None
    if head is not None:
        hs = (float(head[0][0]), float(head[0][1]))
        flat += list(head[1])
    if front is not None:
        fs = (float(front[0][0]), float(front[0][1]))
        flat += list(front[1])
    return _HalfStackFn.apply(x, tuple(specs), _Mode(precision), torch.is_grad_enabled(), pack_cache, hs, fs, int(pool), *flat)


class _HalfConvFn(torch.autograd.Function):
    """CausalConv1d / NonCausalConv1d / 1x1 Conv1d (modules/conv_ops.py:39-44, 73-79) on the half-precision kernels
    (wn_hconv_*): dense fp32 in and out like functional.dilated_conv, half series and MFMAs inside.  Used by the conv
    modules and the output stacks of a model that set_precision switched to a half mode."""

    @staticmethod
    @_on_device_of_first_tensor
    def forward(ctx, x, weight, bias, dilation, causal, mode, grad_enabled):
        lib = _lib.load()
        _require_device(x, "input")
        _require_device(weight, "weight")
        _flags.WATCH.poll()
        B, Ci, L = x.shape
        Co, Ci_w, k = weight.shape
        if Ci_w != Ci:
            raise RuntimeError("wavenet_speech_amd: input has %d channels, conv expects %d" % (Ci, Ci_w))
        dev = x.device
        reach = max(abs(o) for o in _lib.tap_offsets(k, dilation, causal))
        layout = HalfLayout(L, reach)
        shape = _lib.ConvShape(B, L, Ci, Co, k, int(dilation), int(bool(causal)), layout.ld, layout.halo)
        training = bool(grad_enabled) and any(ctx.needs_input_grad)
        c = _hcall(lib, B, layout, dev, mode)                 # (c.rs: inputs are stored as x / 16 like the residual stream)
        w = weight.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        packed = _pack_hconv(c, shape, w, b)
        xin = _lease(c, Ci)
        _load(lib, mode, x.detach().contiguous(), xin, layout, c.rs, None, c.flag)
        y = torch.empty(B, Co, L, dtype=torch.float32, device=dev)
        _lib.check(lib.wn_hconv_forward(ctypes.byref(shape), mode.code, _p(packed), _p(xin), _p(y), _stream()), "wn_hconv_forward")
        _flags.WATCH.note(c.flag, _OVERFLOW_MSG % "input of a conv", at_once=not training)
        if training:
            ctx.saved = (xin, packed, shape)
        ctx.layout, ctx.dims, ctx.has_bias, ctx.mode, ctx.rs = layout, (B, Ci, Co, k), bias is not None, mode, c.rs
        return y

    @staticmethod
    @once_differentiable
    @_on_device_of_first_tensor
    def backward(ctx, d_y):
        lib = _lib.load()
        _flags.WATCH.poll()
        xin, packed, shape = ctx.saved
        layout, mode = ctx.layout, ctx.mode
        B, Ci, Co, k = ctx.dims
        dev = d_y.device
        d_y = d_y.contiguous()
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if mode.dtype == torch.float16 else None
        dyn, dyn_inv = _grad_scale(d_y, mode)
        dy = _hlease(mode, B, Co, layout, dev)
        _load(lib, mode, d_y, dy, layout, 1.0, dyn, flag)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(B, Ci, layout.length, dtype=torch.float32, device=dev)
            _lib.check(lib.wn_hconv_backward_data(ctypes.byref(shape), mode.code, _p(packed), _p(dy), _p(dx), _p(dyn_inv), _stream()),
                       "wn_hconv_backward_data")
        dw, db = _hconv_wgrad(_HCall(lib, B, layout, dev, mode, flag, ctx.rs), shape, xin, dy, (Co, Ci, k), ctx.has_bias, dyn_inv)
        _flags.WATCH.note(flag, _OVERFLOW_MSG % "gradient of a conv", at_once=False)
        ctx.saved = None
        return dx, dw, db, None, None, None, None


def conv(x, weight, bias, dilation, causal, precision):
    """functional.dilated_conv in a half-precision mode ("f16x3" / "f16" / "bf16")"""
    if precision not in ("f16x3", "f16", "bf16"):
        raise ValueError("unknown precision %r" % (precision,))
    return _HalfConvFn.apply(x, weight, bias, int(dilation), bool(causal), _Mode(precision), torch.is_grad_enabled())

