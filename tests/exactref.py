"""Exact references for the fp32 and f16x3 kernels: inputs on a dyadic grid, results that no summation order can change.

Every operand is a small integer times a power of two, and every product satisfies  sum |w| |x| < 2^24 units of its result grid
(the finest grid that holds every term).  Every partial sum of such a product, in any order, over any tiling, split-K slab or
accumulate pass, is then an integer number of units below 2^24: exactly representable in fp32.  The true result, computed here in
fp64, is what a correct kernel returns bit for bit, so the GPU tests compare with torch.equal and one wrong element of any
size fails.

The gate joins in through saturation.  The kernels' tanh and sigmoid are built from exp2 and rcp (csrc/wn_gemm.hip, wn_half_dev.h):
tanh(0) = 0, tanh(x) = +-1 once exp(-2|x|) < 2^-24, sigmoid(x) = 1 for x >= 17, 0 for x <= -89 (exp2 overflows, rcp(inf) = 0), and
sigmoid(0) = rcp(2).  With every gate pre-activation an integer multiple of Q = 128, tanh is in {-1, 0, 1}, sigmoid in {0, 1/2, 1},
z and the saved sigmoid are exact, and so is the backward rule the kernels implement (t = z / s, da = dz (s - z t),
dg = dz z (1 - s)): da in {0, dz/2, dz}, dg in {0, +-dz/4}.  LeakyReLU with a dyadic slope (0.25, 0.5) keeps the grid.

How gradients keep inside 24 bits through a stack.  A gate pre-activation on the grid Q from activations on the grid 1/2 needs
gate weights that are multiples of 2 Q, so the backward path through a gate (dz -> da, dg -> dx) multiplies magnitudes by 256 and
divides the grid by 4, while the path beside it (residual_proj, the skip projection) does neither: every block whose gate passes
a gradient costs about ten of the 24 bits.  A stack case therefore draws gates that take all nine (tanh, sigmoid) pairs in its
TOP TWO blocks -- the top block's input gradient is pure gate path, so the chain below it gets a non-zero dr at all, and the
block under it passes that gradient through a second gate (22.7 bits in the largest case) -- and saturates the block below
them (da = dg = 0 there, asserted as exact zeros).  The single-block cases exercise the nine pairs at every shape.

assert_exact(case) proves the conditions for a case on the CPU; the GPU tests call it before they touch the device, and
tests/test_exactref.py runs it over the whole case table and pins every reference here to the fp64 oracle.

Imports torch, numpy and the oracle; nothing from the package."""
import functools

import numpy as np
import torch

from oracle import wavenet_oracle as O

DT = torch.float64
Q = 128.0                # every gate pre-activation is a multiple of this (>= 89: sigmoid(-Q) is exactly 0)
LIMIT = float(2 ** 24)
RS = 1.0 / 16            # wn_hseries_residual_scale(): the half series of a conv's input holds x / 16
WS = 256.0               # kWeightScale: packed weights hold 256 w / (the scale of their input)
GRAD_TARGET = 0.25       # functional_half.GRAD_TARGET
NINE = [(t, s) for t in (-1.0, 0.0, 1.0) for s in (0.0, 0.5, 1.0)]


# ------------------------------------------------------------------------------------------------------------------
# grids
# ------------------------------------------------------------------------------------------------------------------
def unit(t):
    """the largest power of two that divides every element of t (1.0 for an all-zero tensor)"""
    v = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64).ravel()
    v = v[v != 0]
    if v.size == 0:
        return 1.0
    assert np.isfinite(v).all()
    m, e = np.frexp(v)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mi & -mi).astype(np.float64))
    return float(2.0 ** np.min(e - 53 + tz))


def is_fp32(t):
    return bool(torch.equal(t.float().double(), t))


# ------------------------------------------------------------------------------------------------------------------
# seeded generators
# ------------------------------------------------------------------------------------------------------------------
def rng_of(*seed):
    return np.random.RandomState([int(s) & 0x7FFFFFFF for s in seed])


def dyadic(rng, shape, bits, exp=0, density=1.0):
    """integers of at most `bits` significant bits (|n| < 2^bits) times 2^exp, a fraction `density` of them non-zero"""
    top = 2 ** bits - 1
    n = rng.randint(-top, top + 1, size=shape).astype(np.float64)
    if density < 1.0:
        n *= rng.random_sample(shape) < density
    return torch.from_numpy(n * 2.0 ** exp)


def two_plane(rng, shape, exp=0):
    """odd integers of 12 to 13 significant bits times 2^exp: fp16 (11 bits) cannot hold them, hi + lo of the f16x3 split can"""
    n = (rng.randint(2 ** 10, 2 ** 12, size=shape) * 2 + 1).astype(np.float64)
    n *= rng.choice([-1.0, 1.0], size=shape)
    return torch.from_numpy(n * 2.0 ** exp)


def signed_sparse(rng, rows, cols, per_row, scale=1.0):
    """[rows, cols] with entries in {-1, 0, 1} * scale, about `per_row` non-zeros in a row and at least one: weights of the
    residual chain that keep magnitudes from growing block to block"""
    m = np.zeros((rows, cols))
    for r in range(rows):
        idx = rng.choice(cols, size=min(cols, per_row), replace=False)
        m[r, idx] = rng.choice([-1.0, 1.0], size=idx.size)
    return torch.from_numpy(m * scale)


def time_sparse(rng, B, C, L, bits, col_density, density=1.0, exp=0):
    """a cotangent that is non-zero in a fraction of the time columns only, the first and last column and both sides of every
    32- and 128-step boundary among them"""
    t = dyadic(rng, (B, C, L), bits, exp, density)
    keep = rng.random_sample((B, 1, L)) < col_density
    for e in [0, L - 1] + [c + o for c in range(32, L, 32) for o in (-1, 0)]:
        keep[:, :, e] = True
    return t * torch.from_numpy(keep.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------
# products with their accumulation bound
# ------------------------------------------------------------------------------------------------------------------
class Rec(list):
    """the products of a case.  With `hscale` set the case is an f16x3 one: every term that names the storage scales of its
    operands -- (fn, operands, scales), "dyn" standing for the call's gradient scale `dyn` -- is also checked as the half kernels
    form it (_three_planes)."""
    hscale = False
    dyn = None

    def __init__(self):
        list.__init__(self)
        self.half = []


def _three_planes(rec, name, fn, ops, scales):
    """one term as the f16x3 kernels form it: each operand times its scale in two fp16 planes, hi hi + hi lo + lo hi in fp32"""
    scales = [rec.dyn if s == "dyn" else s for s in scales]
    planes = [split16(o, s) for o, s in zip(ops, scales)]
    for i, ((h, l), o, s) in enumerate(zip(planes, ops, scales)):
        ok = bool(torch.isfinite(h).all()) and torch.equal(h + l, o * s)
        rec.half.append((name, ok, "operand %d leaves fp16's range or its two planes do not hold it" % i))
    if len(ops) == 1:                                       # row sums: both planes are summed
        (h, l), = planes
        rec.append((name + " (planes)", float(fn(h.abs() + l.abs()).max()), min(unit(h), unit(l))))
        return
    (ah, al), (bh, bl) = planes
    got = _acc(rec, name + " (planes)", [(fn, (ah, bh)), (fn, (ah, bl)), (fn, (al, bh))]) / (scales[0] * scales[1])
    rec.half.append((name, torch.equal(got, fn(*ops)), "the three-product result differs from the integer result"))
    rec.half.append((name, float(fn(al.abs(), bl.abs()).abs().max()) == 0.0, "the omitted lo lo product is not zero"))


def _acc(rec, name, terms, add=()):
    """sum of fn(*operands) over `terms` plus the tensors in `add` (biases); records (name, max sum of |.| |.|, unit)"""
    val = bound = None
    u = None
    if getattr(rec, "hscale", False):
        for t in terms:
            if len(t) == 3:
                _three_planes(rec, name, *t)
    for fn, ops in [t[:2] for t in terms]:
        v = fn(*ops)
        b = fn(*[o.abs() for o in ops])
        val = v if val is None else val + v
        bound = b if bound is None else bound + b
        if any(float(o.abs().max()) == 0.0 for o in ops if o.numel()):
            continue                                   # an all-zero operand: no term, no grid
        tu = 1.0
        for o in ops:
            tu *= unit(o)
        u = tu if u is None else min(u, tu)
    for a in add:
        val = val + a
        bound = bound + a.abs()
        if float(a.abs().max()) > 0.0:
            u = unit(a) if u is None else min(u, unit(a))
    u = 1.0 if u is None else u
    rec.append((name, float(bound.max()) if bound.numel() else 0.0, u))
    return val


def _mm(w, x):          # [O, C] x [B, C, L] -> [B, O, L]
    return torch.einsum("oc,bcl->bol", w, x)


def _mmT(w, g):         # [O, C]^T x [B, O, L] -> [B, C, L]
    return torch.einsum("oc,bol->bcl", w, g)


def _outer(g, x):       # sum over batch and time: [B, O, L] x [B, C, L] -> [O, C]
    return torch.einsum("bol,bcl->oc", g, x)


def _rowsum(g):
    return g.sum((0, 2))


def _col(b):
    return b.view(1, -1, 1)


def conv_forward(rec, name, x, w, b, d, causal):
    offs = O.tap_offsets(w.shape[2], d, causal)
    terms = [(lambda w_, x_, j=j, off=off: _mm(w_[:, :, j], O.shifted(x_, off)), (w, x), (WS / RS, RS)) for j, off in enumerate(offs)]
    bias = [] if b is None else [_col(b).expand(x.shape[0], -1, x.shape[2])]
    return _acc(rec, name, terms, bias)


def conv_backward(rec, name, x, w, dy, d, causal, has_bias=True, want_dx=True):
    """(dx, dw, db) of y = conv(x, w) + b for the cotangent dy"""
    k = w.shape[2]
    offs = O.tap_offsets(k, d, causal)
    dx = None
    if want_dx:
        dx = _acc(rec, name + ".dx", [(lambda w_, g_, j=j, off=off: O.shifted(_mmT(w_[:, :, j], g_), -off), (w, dy), (WS, "dyn"))
                                      for j, off in enumerate(offs)])
    dw = torch.stack([_acc(rec, "%s.dw[tap %d]" % (name, j),
                           [(lambda g_, x_, off=off: _outer(g_, O.shifted(x_, off)), (dy, x), ("dyn", RS))])
                      for j, off in enumerate(offs)], 2)
    db = _acc(rec, name + ".db", [(_rowsum, (dy,), ("dyn",))]) if has_bias else None
    return dx, dw, db


# ------------------------------------------------------------------------------------------------------------------
# the residual block with the three-valued gate
# ------------------------------------------------------------------------------------------------------------------
def gate3(a, g):
    """(tanh, sigmoid) of pre-activations that are multiples of Q, as the kernels' exp2 / rcp forms give them"""
    return torch.sign(a), torch.where(g > 0, torch.ones_like(g), torch.where(g < 0, torch.zeros_like(g), torch.full_like(g, 0.5)))


def block_forward(rec, name, x, p, d, causal, gates):
    a = conv_forward(rec, name + ".a", x, p["conv_tanh.conv1d.weight"], p["conv_tanh.conv1d.bias"], d, causal)
    g = conv_forward(rec, name + ".g", x, p["conv_sigmoid.conv1d.weight"], p["conv_sigmoid.conv1d.bias"], d, causal)
    gates.append((name, a, g))
    ta, sg = gate3(a, g)
    z = ta * sg
    Wr, Wk, Wp = p["conv1x1_residual.weight"][:, :, 0], p["conv1x1_skip.weight"][:, :, 0], p["residual_proj.weight"]
    B, _, L = x.shape
    r = _acc(rec, name + ".r", [(_mm, (Wr, z), (WS, 1.0)), (_mm, (Wp, x), (WS / RS, RS))],
             [_col(p["conv1x1_residual.bias"] + p["residual_proj.bias"]).expand(B, -1, L)])
    return r, ta, sg, z


def block_backward(rec, name, x, p, d, causal, sg, z, dr, ds, w_skip, want_dx=True):
    """the rule of csrc/wn_gemm.hip: t = z / s, da = dz (s - z t), dg = dz z (1 - s).  dr None: the residual output is unused
    (conv1x1_residual and residual_proj then get no gradient).  w_skip: the matrix that made the skip output (conv1x1_skip, or
    the folded bottleneck x skip product in a stack); its gradient is returned under "skip.weight" / "skip.bias"."""
    Wt, Ws = p["conv_tanh.conv1d.weight"], p["conv_sigmoid.conv1d.weight"]
    Wr, Wp = p["conv1x1_residual.weight"][:, :, 0], p["residual_proj.weight"]
    terms = [(_mmT, (w_skip, ds), (WS, "dyn"))] + ([(_mmT, (Wr, dr), (WS, "dyn"))] if dr is not None else [])
    dz = _acc(rec, name + ".dz", terms)
    t = torch.where(sg > 0, z / torch.where(sg > 0, sg, torch.ones_like(sg)), torch.zeros_like(z))
    da = dz * (sg - z * t)
    dg = dz * z * (1 - sg)
    offs = O.tap_offsets(Wt.shape[2], d, causal)
    dx = None
    if want_dx:
        terms = [(_mmT, (Wp, dr), (WS, "dyn"))] if dr is not None else []
        for j, off in enumerate(offs):
            terms.append((lambda w_, g_, j=j, off=off: O.shifted(_mmT(w_[:, :, j], g_), -off), (Wt, da), (WS, "dyn")))
            terms.append((lambda w_, g_, j=j, off=off: O.shifted(_mmT(w_[:, :, j], g_), -off), (Ws, dg), (WS, "dyn")))
        dx = _acc(rec, name + ".dx", terms)
    grads = {}
    for key, gg in (("conv_tanh", da), ("conv_sigmoid", dg)):
        grads[key + ".conv1d.weight"] = torch.stack(
            [_acc(rec, "%s.d%s[tap %d]" % (name, key, j), [(lambda g_, x_, off=off: _outer(g_, O.shifted(x_, off)), (gg, x), ("dyn", RS))])
             for j, off in enumerate(offs)], 2)
        grads[key + ".conv1d.bias"] = _acc(rec, "%s.d%s.bias" % (name, key), [(_rowsum, (gg,), ("dyn",))])
    grads["skip.weight"] = _acc(rec, name + ".dskip", [(_outer, (ds, z), ("dyn", 1.0))])
    grads["skip.bias"] = _acc(rec, name + ".dskip.bias", [(_rowsum, (ds,), ("dyn",))])
    if dr is not None:
        grads["conv1x1_residual.weight"] = _acc(rec, name + ".dres", [(_outer, (dr, z), ("dyn", 1.0))]).unsqueeze(2)
        grads["residual_proj.weight"] = _acc(rec, name + ".dproj", [(_outer, (dr, x), ("dyn", RS))])
        grads["conv1x1_residual.bias"] = grads["residual_proj.bias"] = _acc(rec, name + ".dres.bias", [(_rowsum, (dr,), ("dyn",))])
    return dx, da, dg, grads


def draw_block(rng, ci, co, ms, k, mode, in_unit=1.0, res_scale=1.0):
    """the ten tensors of a block whose input lies on the grid `in_unit`.  mode "saturated": every gate pre-activation is an odd
    multiple of Q (weights give even multiples, biases odd ones); "mixed": multiples of Q that include 0."""
    gw = Q / in_unit
    if mode == "saturated":
        wscale, biases = 2 * gw, [-3.0, -1.0, 1.0, 3.0]
    else:
        assert mode == "mixed"
        wscale, biases = gw, [-1.0, 0.0, 0.0, 1.0]
    p = {}
    for key in ("conv_tanh", "conv_sigmoid"):
        p[key + ".conv1d.weight"] = signed_sparse(rng, co, ci * k, 2, wscale).view(co, ci, k).contiguous()
        p[key + ".conv1d.bias"] = torch.from_numpy(rng.choice(biases, size=co) * Q)
    p["conv1x1_residual.weight"] = signed_sparse(rng, co, co, 3, res_scale).unsqueeze(2)
    p["conv1x1_residual.bias"] = dyadic(rng, (co,), 2) * res_scale
    p["conv1x1_skip.weight"] = signed_sparse(rng, ms, co, 3).unsqueeze(2)
    p["conv1x1_skip.bias"] = dyadic(rng, (ms,), 2)
    p["residual_proj.weight"] = signed_sparse(rng, co, ci, 1)
    p["residual_proj.bias"] = dyadic(rng, (co,), 1) * res_scale
    return {k_: p[k_] for k_ in O.BLOCK_KEYS}


def pairs_seen(ta, sg):
    return set(zip(ta.flatten().tolist(), sg.flatten().tolist()))


class Case(object):
    """inputs (fp64, exactly representable in fp32), the exact results under .ref, every product's bound under .products and
    every gate pre-activation under .gates"""

    def __init__(self, **kw):
        self.products, self.gates, self.ref = Rec(), [], {}
        self.__dict__.update(kw)


def assert_exact(case):
    """every product's sum |w| |x| stays below 2^24 units of its grid, every gate pre-activation is a multiple of Q, every
    reference tensor is exactly representable in fp32, and (f16x3) the emulated split reproduces the integer result"""
    assert case.products
    for name, bound, u in case.products:
        assert bound < LIMIT * u, "%s: sum |w||x| = %g is %.3g units of %g (limit 2^24)" % (name, bound, bound / u, u)
    for name, a, g in case.gates:
        for what, t in (("a", a), ("g", g)):
            assert bool(((t / Q) == torch.round(t / Q)).all()), "%s.%s is not a multiple of %g" % (name, what, Q)
    for key, t in case.ref.items():
        assert is_fp32(t), "%s is not exactly representable in fp32" % key
    for name, ok, why in case.products.half:
        assert ok, "%s: %s" % (name, why)


# ------------------------------------------------------------------------------------------------------------------
# case tables of tests/test_gpu_exact.py  (B, Ci, Co, k, d, causal, L)
# ------------------------------------------------------------------------------------------------------------------
CONV_CASES = [
    (2, 40, 24, 2, 1, True, 130),      # ragged row slab, cp8 padding, a full column tile and a 2-column clip
    (1, 8, 8, 2, 2, True, 1),          # one time step
    (2, 9, 33, 3, 4, False, 129),      # non-causal, odd everything
    (3, 1, 65, 8, 3, True, 127),       # WN_MAX_TAPS
    (2, 33, 40, 2, 200, True, 128),    # dilation beyond L: tap 0 sees padding only and its dw is exactly 0; one tile exactly
    (2, 24, 24, 1, 1, True, 257),      # k = 1; 18 wgrad chunks: 16 splits, the XCD-mapped placement
    (1, 300, 260, 2, 3, True, 40),     # more than 256 channels: several slabs and wgrad tiles
    (2, 16, 16, 2, 1, False, 256),     # even-k autopad where the padded layout equals the dense one
]
CONV_NO_BIAS = (2, 40, 24, 2, 1, True, 130)
HALF_CONV_CASES = [CONV_CASES[0], CONV_CASES[1], CONV_CASES[2], CONV_CASES[4], (2, 256, 256, 1, 1, True, 512),
                   (2, 40, 72, 2, 3, True, 257)]
# which operand needs both planes of the split (the other two are fp16-exact with few bits)
HALF_CLASSES = ["none", "x", "w", "dy"]
# (Ci, Co, k, d, causal, L, B)
BLOCK_CASES = [(40, 40, 2, 1, True, 130, 2), (33, 65, 3, 5, False, 127, 3), (8, 8, 2, 2, True, 1, 1), (300, 260, 2, 3, True, 40, 1),
               (24, 40, 2, 64, True, 33, 2)]
GATE_MODES = ["saturated", "mixed"]
C, MS, IN, B = 40, 24, 11, 2           # the stacks of tests/test_gpu_f32_series.py
STACKS = {"three_k2": [(C, C, 2, 1), (C, C, 2, 2), (C, C, 2, 4)], "one_k3": [(C, C, 3, 2)]}
LENGTHS = [130, 128, 5]
NET_CASES = [("three_k2", 130), ("one_k3", 5)]
SLOPES = (0.25, 0.5)
HALF_GRID = 128.0        # f16x3 stack: the residual stream lies on this grid (packed gate weights must stay below 16)
ZERO_ROW = 7


def _seed(*case):
    return [int(v) for v in case]


@functools.lru_cache(maxsize=None)
def conv_case(case, bias=True):
    Bn, ci, co, k, d, causal, L = case
    rng = rng_of(1, *_seed(*case))
    c = Case(kind="conv", case=case, d=d, causal=causal)
    c.x = dyadic(rng, (Bn, ci, L), 4, -1, 0.8)
    c.w = dyadic(rng, (co, ci, k), 3, -2, 0.7)
    c.b = dyadic(rng, (co,), 5, -3) if bias else None
    c.dy = dyadic(rng, (Bn, co, L), 3, -1, 0.8)
    c.ref["y"] = conv_forward(c.products, "y", c.x, c.w, c.b, d, causal)
    c.ref["dx"], c.ref["dw"], db = conv_backward(c.products, "conv", c.x, c.w, c.dy, d, causal, bias)
    if bias:
        c.ref["db"] = db
    return c


# ------------------------------------------------------------------------------------------------------------------
# f16x3: the split as the code defines it, in numpy float16
# ------------------------------------------------------------------------------------------------------------------
def split16(t, scale):
    """(hi, lo) planes of t * scale: hi = fp16(v), lo = fp16(v - hi)  (csrc/wn_half.h)"""
    v = t.numpy() * scale
    with np.errstate(over="ignore"):
        hi = v.astype(np.float16).astype(np.float64)
        lo = (v - hi).astype(np.float16).astype(np.float64)
    return torch.from_numpy(hi), torch.from_numpy(lo)


def grad_scale(dy):
    """wn_grad_scale: the power of two that puts max |dy| in (GRAD_TARGET / 2, GRAD_TARGET]"""
    amax = max(float(dy.abs().max()), 1e-30)
    return 2.0 ** min(100.0, max(-100.0, float(np.floor(np.log2(GRAD_TARGET / amax)))))


@functools.lru_cache(maxsize=None)
def half_conv_case(case, cls):
    """a conv whose f16x3 evaluation is exact: `cls` names the one operand that needs both planes"""
    Bn, ci, co, k, d, causal, L = case
    rng = rng_of(2, HALF_CLASSES.index(cls), *_seed(*case))
    c = Case(kind="half_conv", case=case, cls=cls, d=d, causal=causal)
    few = 0.5 if max(ci * k, co * k) <= 64 else 0.25                       # density of the few-bit operands
    c.x = two_plane(rng, (Bn, ci, L), -6) if cls == "x" else dyadic(rng, (Bn, ci, L), 2 if cls == "none" else 1, 0, few)
    c.w = two_plane(rng, (co, ci, k), -13) if cls == "w" else dyadic(rng, (co, ci, k), 2 if cls == "none" else 1, -2, few)
    c.b = dyadic(rng, (co,), 3, -2)
    c.dy = two_plane(rng, (Bn, co, L), -10) if cls == "dy" else dyadic(rng, (Bn, co, L), 2, 0, few) * 0.75
    c.products.hscale = True
    c.products.dyn = c.dyn = grad_scale(c.dy)
    # forward: weights packed at WS / RS against x stored at RS, the fp32 bias starts the accumulator; backward data: weights at WS
    # against dy at the call's gradient scale; weight gradients: dy against x; the bias gradient: row sums of both planes of dy
    c.ref["y"] = conv_forward(c.products, "y", c.x, c.w, c.b, d, causal)
    c.ref["dx"], c.ref["dw"], c.ref["db"] = conv_backward(c.products, "conv", c.x, c.w, c.dy, d, causal)
    return c


# ------------------------------------------------------------------------------------------------------------------
# block and stack cases
# ------------------------------------------------------------------------------------------------------------------
def _steer(p, x, d, causal):
    """one gate element per channel (B L = 1): set each bias so that the channels walk through the nine (tanh, sigmoid) pairs"""
    for key, col in (("conv_tanh", 0), ("conv_sigmoid", 1)):
        w = p[key + ".conv1d.weight"]
        pre = conv_forward([], "", x, w, None, d, causal)[0, :, 0]
        want = torch.tensor([(NINE[i % 9][col] if col == 0 else 2 * NINE[i % 9][col] - 1) for i in range(w.shape[0])], dtype=DT)
        p[key + ".conv1d.bias"] = want * Q - pre


@functools.lru_cache(maxsize=None)
def block_case(case, mode):
    ci, co, k, d, causal, L, Bn = case
    for attempt in range(64):
        rng = rng_of(3, GATE_MODES.index(mode), attempt, *_seed(*case))
        c = Case(kind="block", case=case, mode=mode, d=d, causal=causal)
        c.x = dyadic(rng, (Bn, ci, L), 2, 0, 0.7)
        c.p = draw_block(rng, ci, co, co, k, mode)
        if mode == "mixed" and Bn * L == 1:
            _steer(c.p, c.x, d, causal)
        c.dr, c.ds = dyadic(rng, (Bn, co, L), 2, 0, 0.8), dyadic(rng, (Bn, co, L), 2, -1, 0.8)
        r, ta, sg, z = block_forward(c.products, "block", c.x, c.p, d, causal, c.gates)
        c.pairs = pairs_seen(ta, sg)
        c.want_pairs = min(9, Bn * L * co) if mode == "mixed" else 0
        if len(c.pairs) >= c.want_pairs:
            break
    Wk = c.p["conv1x1_skip.weight"][:, :, 0]
    s = _acc(c.products, "block.s", [(_mm, (Wk, z))], [_col(c.p["conv1x1_skip.bias"]).expand(Bn, -1, L)])
    dx, da, dg, grads = block_backward(c.products, "block", c.x, c.p, d, causal, sg, z, c.dr, c.ds, Wk)
    grads["conv1x1_skip.weight"] = grads.pop("skip.weight").unsqueeze(2)
    grads["conv1x1_skip.bias"] = grads.pop("skip.bias")
    c.ref.update({"r": r, "s": s, "dx": dx, "sg": sg, "z": z, "da": da, "dg": dg})
    c.ref.update(grads)
    return c


def _leaky(pre, slope):
    return torch.where(pre > 0, pre, pre * slope)


def _mask(pre, slope):
    return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))


@functools.lru_cache(maxsize=None)
def stack_case(stack, L, net=False, half=False):
    """net False: the stack alone (modules.block.run_stack on a dense input, result skips_sum); True: a WaveNet -- entry conv on a
    one-hot input, the stack, LeakyReLU(0.25), 1x1, LeakyReLU(0.5), 1x1 -- whose row ZERO_ROW of skips_sum is exactly 0.
    State-dict keys are the model's.  The gates of the top two blocks take all nine value pairs, the block below is saturated."""
    for attempt in range(64):
        c = _stack_case(stack, L, net, attempt, half)
        if len(c.pairs) == 9 and (not net or float(c.ref["bottlenecks.0.bias"][ZERO_ROW].abs()) > 0):
            break
    return c


def _stack_case(stack, L, net, attempt, half=False):
    layers = STACKS[stack]
    n = len(layers)
    if True:
        rng = rng_of(4, sorted(STACKS).index(stack), L, int(net) + 2 * int(half), attempt)
        c = Case(kind="net" if net else "stack", stack=stack, L=L, layers=layers, pairs=None)
        sd, rec = {}, c.products
        assert not (net and half)
        rec.hscale = half
        mixed_from = n - 1 if half else n - 2
        if net:
            c.levels = torch.from_numpy(rng.randint(0, IN, size=(B, L)))
            c.x = O.one_hot_encoding(c.levels, IN).double()
            sd["entry_conv1d.conv1d.weight"] = dyadic(rng, (C, IN, 2), 2, 0, 0.5)
            sd["entry_conv1d.conv1d.bias"] = dyadic(rng, (C,), 1)
            cur = conv_forward(rec, "entry", c.x, sd["entry_conv1d.conv1d.weight"], sd["entry_conv1d.conv1d.bias"], 1, True)
        else:
            c.x = cur = dyadic(rng, (B, C, L), 2, 0, 0.7) * (HALF_GRID if half else 1.0)
        xs, saved, S_terms, bias_total, wfs = [], [], [], torch.zeros(MS, dtype=DT), []
        for l, (ci, co, k, d) in enumerate(layers):
            pre = "convolutions.%d." % l
            if half:
                p = draw_block(rng, ci, co, co, k, "mixed" if l >= mixed_from else "saturated", HALF_GRID, HALF_GRID)
            else:
                p = draw_block(rng, ci, co, co, k, "mixed" if l >= mixed_from else "saturated", 1.0 if l == 0 else 0.5)
            wb = signed_sparse(rng, MS, co, 2)
            bb = dyadic(rng, (MS,), 2)
            if net:
                wb[ZERO_ROW] = 0
                bb[ZERO_ROW] = 0
            sd.update({pre + k_: v for k_, v in p.items()})
            sd["bottlenecks.%d.weight" % l], sd["bottlenecks.%d.bias" % l] = wb.unsqueeze(2), bb
            wk, bk = p["conv1x1_skip.weight"][:, :, 0], p["conv1x1_skip.bias"]
            wf = _acc(rec, "fold%d.w" % l, [(torch.matmul, (wb, wk))])               # modules.block.fold_bottlenecks, on the device
            bf = _acc(rec, "fold%d.b" % l, [(torch.mv, (wb, bk))], [bb])
            r, ta, sg, z = block_forward(rec, "block%d" % l, cur, p, d, True, c.gates)
            if l >= mixed_from and (c.pairs is None or len(pairs_seen(ta, sg)) < len(c.pairs)):
                c.pairs = pairs_seen(ta, sg)          # of the unsaturated blocks, the one that shows the fewest pairs
            xs.append(cur)
            saved.append((p, d, sg, z, wf, wb, wk, bk))
            S_terms.append((_mm, (wf, z), (WS, 1.0)))
            bias_total = bias_total + bf
            cur = r
    rec.append(("bias_total", float(sum(s_[4].abs().max() for s_ in saved)), 1.0))
    S = _acc(rec, "skips_sum", S_terms, [_col(bias_total).expand(B, -1, L)])
    c.ref["skips_sum"] = S
    g = rng_of(5, sorted(STACKS).index(stack), L, int(net), attempt)
    if net:
        s1, s2 = SLOPES
        for i in (1, 3):
            sd["output_stack.%d.weight" % i] = signed_sparse(g, MS, MS, 3).unsqueeze(2)
            sd["output_stack.%d.bias" % i] = dyadic(g, (MS,), 2)
        sd["output_stack.1.weight"][0, ZERO_ROW, 0] = 1.0                    # the zero row of skips_sum feeds the head
        W1, W2 = sd["output_stack.1.weight"][:, :, 0], sd["output_stack.3.weight"][:, :, 0]
        h0 = _leaky(S, s1)
        pre1 = _acc(rec, "head.1", [(_mm, (W1, h0))], [_col(sd["output_stack.1.bias"]).expand(B, -1, L)])
        h1 = _leaky(pre1, s2)
        y = _acc(rec, "head.3", [(_mm, (W2, h1))], [_col(sd["output_stack.3.bias"]).expand(B, -1, L)])
        c.slopes = {"output_stack.0": _mask(S, s1), "output_stack.2": _mask(pre1, s2)}
        c.zero_row_is_zero = float(S[:, ZERO_ROW].abs().max()) == 0.0
        c.ref["forward"] = y
        c.cot = time_sparse(g, B, MS, L, 2, 1.0, 0.7)
        _, dw2, db2 = conv_backward(rec, "head.3", h1, W2.unsqueeze(2), c.cot, 1, True, want_dx=False)
        dh1 = _acc(rec, "head.3.dx", [(_mmT, (W2, c.cot))]) * c.slopes["output_stack.2"]
        _, dw1, db1 = conv_backward(rec, "head.1", h0, W1.unsqueeze(2), dh1, 1, True, want_dx=False)
        dS = _acc(rec, "head.1.dx", [(_mmT, (W1, dh1))]) * c.slopes["output_stack.0"]
        c.ref.update({"output_stack.1.weight": dw1, "output_stack.1.bias": db1, "output_stack.3.weight": dw2,
                      "output_stack.3.bias": db2})
    else:
        c.ref["forward"] = S
        c.cot = dS = time_sparse(g, B, MS, L, 2, 1.0, 0.7)
        rec.dyn = c.dyn = grad_scale(c.cot)
    dr = None
    for l in range(n - 1, -1, -1):
        p, d, sg, z, wf, wb, wk, bk = saved[l]
        pre = "convolutions.%d." % l
        dx, da, dg, grads = block_backward(rec, "block%d" % l, xs[l], p, d, True, sg, z, dr, dS, wf, want_dx=True)
        dwf, dbf = grads.pop("skip.weight"), grads.pop("skip.bias")
        # autograd through the fold: Wf = Wb Wk, bf = Wb bk + bb
        c.ref["bottlenecks.%d.weight" % l] = _acc(rec, "fold%d.dwb" % l, [(lambda a_, b_: a_ @ b_.t(), (dwf, wk)),
                                                                          (torch.outer, (dbf, bk))]).unsqueeze(2)
        c.ref["bottlenecks.%d.bias" % l] = dbf
        c.ref[pre + "conv1x1_skip.weight"] = _acc(rec, "fold%d.dwk" % l, [(lambda a_, b_: a_.t() @ b_, (wb, dwf))]).unsqueeze(2)
        c.ref[pre + "conv1x1_skip.bias"] = _acc(rec, "fold%d.dbk" % l, [(lambda a_, b_: torch.mv(a_.t(), b_), (wb, dbf))])
        c.ref.update({pre + k_: v for k_, v in grads.items()})
        if l < mixed_from:
            assert float(da.abs().max()) == 0.0 and float(dg.abs().max()) == 0.0       # saturated: exact zeros
        c.ref["block%d.dx" % l] = dx
        dr = dx
    if net:
        c.ref["dx0"], c.ref["entry_conv1d.conv1d.weight"], c.ref["entry_conv1d.conv1d.bias"] = conv_backward(
            rec, "entry", c.x, sd["entry_conv1d.conv1d.weight"], dr, 1, True)
    else:
        c.ref["dx0"] = dr
    c.sd = sd
    return c


def first_difference(got, want):
    """(index of the first differing element, got there, wanted there) or None"""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape:
        return ("shape", tuple(got.shape), tuple(want.shape))
    ne = (got != want) | (torch.isnan(got) != torch.isnan(want))
    if not bool(ne.any()):
        return None
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return idx, float(got[idx]), float(want[idx]), int(ne.sum())
