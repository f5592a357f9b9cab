"""fp64 reference of the plain half-precision modes ("bf16", "f16") that knows their storage format.

The models are evaluated in fp64 with torch autograd.  Wherever the half path stores a tensor in the series layout (DESIGN.md
section 3b) the value is rounded to the mode's format, at the power-of-two scale the half path stores it with
(wn_half_api.hip): the packed weights (256 w / the scale of their input), the residual stream and the head / front series
(value / 16), the gate's sigmoid and z (as they are), and on the way back dr, da, dg, dS and the head / front series gradients
(value * s, s the power of two that puts max |cotangent| of the call at GRAD_TARGET, chosen per autograd call as
functional_half._grad_scale does).  The scales are exact, but they decide where fp16 runs out of exponent: an element below
fp16's normal range keeps fewer bits, and so it does here.  Biases stay exact (fp32 on the device).  fmt=None gives the exact
fp64 model through the same code.

Tests compare e_hip = |HIP - exact| with e_fmt = |this reference - exact| in max-norm and RMS (distances()) and require
e_hip <= KAPPA * e_fmt + FLOOR on both (check()): an error the storage format does not explain -- a dropped bias, a tap
weighted wrong, a rounding the format does not have -- makes e_hip grow while e_fmt stays."""
import math

import torch
import torch.nn.functional as F

from oracle import wavenet_oracle as O

DT = torch.float64
KAPPA = 2.0          # bound on e_hip / e_fmt; see DESIGN.md section 2 for the measured ratios
FLOOR = 2e-6         # fp32 accumulation: the part of e_hip that remains where the format rounds nothing
RS = 1.0 / 16        # kResidualScale: residual stream, head and front series
WS = 256.0           # kWeightScale
GRAD_TARGET = 0.25   # functional_half.GRAD_TARGET


def rnd(t, fmt, scale=1.0):
    """t stored at `scale` (t * scale rounded to the format), back in t's dtype and units"""
    if fmt is None:
        return t
    return (t * scale).to(torch.bfloat16 if fmt == "bf16" else torch.float16).to(t.dtype) / scale


class GradScale(object):
    """the dynamic gradient scale of one autograd call of the half path: set by probe() when the call's cotangent arrives"""

    def __init__(self, fmt):
        self.fmt, self.s = fmt, 1.0


class _Probe(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, gs):
        ctx.gs = gs
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        gs = ctx.gs
        if gs.fmt == "f16":          # (bf16 has fp32's exponent range: no scaling, functional_half._grad_scale)
            amax = max(float(g.abs().max()), 1e-30)
            gs.s = 2.0 ** min(100.0, max(-100.0, math.floor(math.log2(GRAD_TARGET / amax))))
        return g, None


def probe(t, gs):
    """the output of an autograd call of the half path: its cotangent sets the call's gradient scale"""
    return t if gs.fmt is None else _Probe.apply(t, gs)


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, fmt, scale, gs):
        ctx.fmt, ctx.gs = fmt, gs
        return rnd(t, fmt, scale) if scale is not None else t.clone()

    @staticmethod
    def backward(ctx, g):
        return (rnd(g, ctx.fmt, ctx.gs.s) if ctx.gs is not None else g), None, None, None


def q(t, fmt, scale=1.0):
    """stored on the way forward at `scale` (the gradient passes straight through)"""
    return t if fmt is None else _Round.apply(t, fmt, scale, None)


def qg(t, gs):
    """the gradient of t is stored on the way back, at the call's gradient scale (the value is unchanged)"""
    return t if gs.fmt is None else _Round.apply(t, gs.fmt, None, gs)


def qq(t, fmt, scale, gs):
    return t if fmt is None else _Round.apply(t, fmt, scale, gs)


class _Gate(torch.autograd.Function):
    """z = tanh(a) sigmoid(g), stored; backward from the stored z and sigmoid (tanh = z / sigmoid), da and dg stored"""

    @staticmethod
    def forward(ctx, a, g, gs):
        fmt = gs.fmt
        sg = rnd(torch.sigmoid(g), fmt)
        z = rnd(torch.tanh(a) * torch.sigmoid(g), fmt)
        ta = torch.where(sg != 0, z / torch.where(sg != 0, sg, torch.ones_like(sg)), torch.tanh(a))
        ctx.save_for_backward(ta, sg, z)
        ctx.gs = gs
        return z

    @staticmethod
    def backward(ctx, dz):
        ta, sg, z = ctx.saved_tensors
        fmt, s = ctx.gs.fmt, ctx.gs.s
        return rnd(dz * sg * (1 - ta * ta), fmt, s), rnd(dz * z * (1 - sg), fmt, s), None


def gate(a, g, gs):
    if gs.fmt is None:
        return torch.tanh(a) * torch.sigmoid(g)
    return _Gate.apply(a, g, gs)


def _mm(w, x):
    return torch.einsum("oc,bcl->bol", w, x)


def block(x, p, d, causal, gs, wf, bf):
    """one residual block on the stored input x; (r before storing, skip output).  wf, bf: the folded bottleneck x skip pair."""
    fmt, wx, wz = gs.fmt, WS / RS, WS          # weights on x (stored / 16) and on z (stored as is)
    Wt, Ws = q(p["conv_tanh.conv1d.weight"], fmt, wx), q(p["conv_sigmoid.conv1d.weight"], fmt, wx)
    a = O.dilated_conv(x, Wt, p["conv_tanh.conv1d.bias"], d, causal)
    g = O.dilated_conv(x, Ws, p["conv_sigmoid.conv1d.bias"], d, causal)
    z = gate(a, g, gs)
    r = (_mm(q(p["conv1x1_residual.weight"][:, :, 0], fmt, wz), z) + p["conv1x1_residual.bias"].view(1, -1, 1)
         + _mm(q(p["residual_proj.weight"], fmt, wx), x) + p["residual_proj.bias"].view(1, -1, 1))
    return r, _mm(q(wf, fmt, wz), z) + bf.view(1, -1, 1)


def stack(x, sd, layers, causal, gs, prefixes, dense_input_grad=True):
    """skips_sum of the residual stack (fp32 on the device: not stored) inside the autograd call `gs`.  prefixes: [(block prefix,
    bottleneck prefix)] per block.  x: the stack's input before it is stored; dense_input_grad: its gradient leaves the stack dense
    (fp32), else stored."""
    fmt = gs.fmt
    cur = q(x, fmt, RS) if dense_input_grad else qq(x, fmt, RS, gs)
    S = None
    for l, ((_ci, _co, _k, d), (bp, kp)) in enumerate(zip(layers, prefixes)):
        p = O.block_params(sd, bp)
        wb = sd[kp + "weight"][:, :, 0]
        wf = wb @ p["conv1x1_skip.weight"][:, :, 0]
        bf = wb @ p["conv1x1_skip.bias"] + sd[kp + "bias"]
        r, s = block(cur, p, d, causal, gs, wf, bf)
        S = s if S is None else S + s
        if l + 1 < len(layers):
            cur = qq(r, fmt, RS, gs)
    return S


def stack_call(x, sd, layers, causal, fmt, prefixes):
    """run_stack without a head: one autograd call whose output is the dense skips_sum (its cotangent stored on the way back)"""
    gs = GradScale(fmt)
    return probe(qg(stack(x, sd, layers, causal, gs, prefixes), gs), gs)


def hconv(x, w, b, fmt):
    """a 1x1 / causal conv on the half convs outside the stack (wn_hconv_*), an autograd call of its own: stored input (/ 16) and
    weights, dense output whose gradient is stored on the way back, dense input gradient"""
    gs = GradScale(fmt)
    return probe(qg(O.dilated_conv(q(x, fmt, RS), q(w, fmt, WS / RS), b, 1, True), gs), gs)


class Pattern(dict):
    """slopes recorded by one evaluation (each LeakyReLU applied as usual, its per-element slope stored under the module's name),
    to be replayed by the others: pass an empty Pattern(negative_slopes) as `slopes`"""

    def __init__(self, negative_slopes):
        super().__init__()
        self.negative_slopes = negative_slopes


def _leaky(x, slopes, key, slope=0.01):
    if isinstance(slopes, Pattern) and key not in slopes:
        ns = slopes.negative_slopes.get(key, slope)
        slopes[key] = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, ns)).detach()
    if slopes is not None and key in slopes:
        return x * slopes[key].to(x.dtype)
    return F.leaky_relu(x, slope)


def stack_and_head(S, sd, prefix, gs, slopes, fused):
    """the end of the stack call and the output block LeakyReLU, 1x1, LeakyReLU, 1x1.  fused: in the series inside the stack call
    (h0, h1 stored / 16, their gradients stored after the LeakyReLU backward, y dense); else the call ends with the dense
    skips_sum and the block runs as two wn_hconv calls with the LeakyReLUs in torch"""
    fmt = gs.fmt
    w1, b1, w2, b2 = (sd[prefix + s] for s in ("1.weight", "1.bias", "3.weight", "3.bias"))
    if not fused:
        S = probe(qg(S, gs), gs)
        h = hconv(_leaky(S, slopes, prefix + "0"), w1, b1, fmt)
        return hconv(_leaky(h, slopes, prefix + "2"), w2, b2, fmt)
    h0 = q(_leaky(qg(S, gs), slopes, prefix + "0"), fmt, RS)
    h1 = q(_leaky(qg(_mm(q(w1[:, :, 0], fmt, WS / RS), h0) + b1.view(1, -1, 1), gs), slopes, prefix + "2"), fmt, RS)
    return probe(qg(_mm(q(w2[:, :, 0], fmt, WS / RS), h1) + b2.view(1, -1, 1), gs), gs)


def _layers_prefixes(layers):
    return [("convolutions.%d." % l, "bottlenecks.%d." % l) for l in range(len(layers))]


def wavenet(signal, sd, layers, fmt, slopes=None, fused_head=True):
    """WaveNet (oracle.wavenet, softmax off) in a plain half mode: entry conv on the half convs, stack, output stack"""
    out = hconv(signal, sd["entry_conv1d.conv1d.weight"], sd["entry_conv1d.conv1d.bias"], fmt)
    gs = GradScale(fmt)
    S = stack(out, sd, layers, True, gs, _layers_prefixes(layers))
    return stack_and_head(S, sd, "output_stack.", gs, slopes, fused_head)


def raw_ctcnet(seq, sd, layers, feature_kwidth, fmt, causal=False, input_dilation=1, input_kwidth=2, slopes=None,
               fused=True):
    """RawCTCNet (oracle.raw_ctcnet, no positions, softmax off) in a plain half mode.  fused: feature layer and output block inside
    the stack call (fusable_front / fusable_head); else on the half convs with the LeakyReLUs in torch"""
    kf = feature_kwidth
    w0, b0, w1, b1 = (sd["feature_layer.%s" % s] for s in ("0.weight", "0.bias", "2.weight", "2.bias"))
    gs = GradScale(fmt)
    if fused:
        # the first conv is an elementwise kernel on the dense signal (fp32); its output f1 and the stack input are stored / 16
        f1 = q(_leaky(qg(F.conv1d(seq, w0, b0, padding=kf - 1), gs), slopes, "feature_layer.1"), fmt, RS)
        x = _leaky(qg(_mm(q(w1[:, :, 0], fmt, WS / RS), f1) + b1.view(1, -1, 1), gs), slopes, "feature_layer.3")
    else:
        x = hconv(F.pad(seq, (0, kf - 1)), w0, b0, fmt)
        x = _leaky(x, slopes, "feature_layer.1")
        x = _leaky(hconv(x, w1, b1, fmt), slopes, "feature_layer.3")
    all_layers = [(None, None, input_kwidth, input_dilation)] + list(layers)
    prefixes = [("input_block.", "input_skip_bottleneck.")] + _layers_prefixes(layers)
    S = stack(x, sd, all_layers, causal, gs, prefixes)
    return stack_and_head(S, sd, "output_block.", gs, slopes, fused)


POOL_MUTANTS = ("window+1", "divisor-1", "start+1", "tail_folded", "grad_not_divided")


def avg_pool(seq, pool, mutant=None):
    """AvgPool1d(pool) of seq [B, C, L] as WaveNetClassifier.mean_pool applies it (no padding, the tail L % pool dropped), in seq's
    dtype.  Autograd of it is the input gradient the device spreads: / pool, broadcast to the window, zero on the dropped tail.
    mutant: one of POOL_MUTANTS -- what a plausible kernel bug would compute instead (the references of the mutant tests)."""
    L = seq.shape[2]
    Lp = L // pool
    if Lp < 1:
        raise RuntimeError("sequence shorter than the pooling window")
    if mutant is None:
        return F.avg_pool1d(seq, pool)
    if mutant == "window+1":           # pool + 1 samples from each window's start (zero beyond the end), their mean
        return F.avg_pool1d(F.pad(seq, (0, pool + 1)), pool + 1, stride=pool)[:, :, :Lp]
    if mutant == "divisor-1":
        assert pool > 1
        return F.avg_pool1d(seq, pool) * (pool / (pool - 1.0))
    if mutant == "start+1":            # every window starts one sample late
        return F.avg_pool1d(F.pad(seq[:, :, 1:], (0, pool)), pool)[:, :, :Lp]
    if mutant == "tail_folded":        # the last window takes the tail with it
        assert L % pool, "no tail to fold"
        last = seq[:, :, (Lp - 1) * pool:].mean(dim=2, keepdim=True)
        return torch.cat([F.avg_pool1d(seq, pool)[:, :, :Lp - 1], last], dim=2)
    if mutant == "grad_not_divided":   # the value of the mean, the gradient of the sum
        total = F.avg_pool1d(seq, pool) * pool
        return (total / pool).detach() + (total - total.detach())
    raise ValueError(mutant)


def wavenet_classifier(seq, sd, layers, pool, fmt, input_dilation=1, input_kwidth=2, slopes=None, fused=True, pool_mutant=None):
    """WaveNetClassifier (oracle.wavenet_classifier, softmax off) in a plain half mode: one autograd call, non-causal.  The pooled
    load sums the window in fp32, multiplies by 1 / (16 pool) and rounds ONCE (hpool_load_kernel): here the fp64 mean stored
    / 16, the un-pooled input not rounded.  The input gradient leaves the stack dense and is spread by pool_unload_kernel, which is
    autograd of the mean.  fused: the output block inside the stack call (fusable_head), else on the half convs."""
    gs = GradScale(fmt)
    x = avg_pool(seq, pool, pool_mutant)
    all_layers = [(None, None, input_kwidth, input_dilation)] + list(layers)
    prefixes = [("input_block.", "input_skip_bottleneck.")] + _layers_prefixes(layers)
    S = stack(x, sd, all_layers, False, gs, prefixes)
    return stack_and_head(S, sd, "output_block.", gs, slopes, fused)


def run(fn, inputs, sd, cot, fmt):
    """fn(*inputs, sd, fmt) in fp64 with autograd: (output, {name: gradient}) with the inputs' gradients under "dx0", "dx1", ..."""
    sd64 = {k: (v.detach().to(DT).requires_grad_(True) if torch.is_tensor(v) and v.is_floating_point() else v)
            for k, v in sd.items()}
    xs = [t.detach().to(DT).requires_grad_(t.requires_grad) for t in inputs]
    y = fn(*xs, sd64, fmt)
    (y * cot.to(DT)).sum().backward()
    grads = {"dx%d" % i: t.grad for i, t in enumerate(xs) if t.grad is not None}
    grads.update({k: v.grad for k, v in sd64.items() if torch.is_tensor(v) and v.grad is not None})
    return y.detach(), grads


def distances(a, ref):
    """(max-norm, RMS) relative distances of a from ref"""
    a, ref = a.detach().to(DT).cpu(), ref.detach().to(DT).cpu()
    d = a - ref
    mx = float(ref.abs().max())
    nr = float(ref.norm())
    return float(d.abs().max()) / (mx if mx > 0 else 1.0), float(d.norm()) / (nr if nr > 0 else 1.0)


def compare(label, hip, fmt_ref, exact, kappa=KAPPA, floor=FLOOR, quiet=False):
    """{tensor name: (e_hip, e_fmt, pass)} for every name of `exact`; prints one line per tensor.  hip / fmt_ref / exact:
    {name: tensor}.  pass = e_hip <= kappa e_fmt + floor in max-norm AND RMS."""
    res = {}
    for k in exact:
        eh, ef = distances(hip[k], exact[k]), distances(fmt_ref[k], exact[k])
        ok = all(h <= kappa * f + floor for h, f in zip(eh, ef))
        res[k] = (eh, ef, ok)
        if not quiet:
            print("%s %-34s e_hip %.2e / %.2e  e_fmt %.2e / %.2e  ratio %.2f / %.2f%s"
                  % (label, k, eh[0], eh[1], ef[0], ef[1], eh[0] / max(ef[0], 1e-30), eh[1] / max(ef[1], 1e-30),
                     "" if ok else "  FAIL"))
    return res


def check(label, hip, fmt_ref, exact, kappa=KAPPA, floor=FLOOR):
    res = compare(label, hip, fmt_ref, exact, kappa, floor)
    bad = {k: (v[0], v[1]) for k, v in res.items() if not v[2]}
    assert not bad, (label, bad)
    return res
