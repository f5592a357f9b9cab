"""What the GPU tests of the model path share (conv, block, stack, WaveNet, RawCTCNet, classifier and the joint step):
the bounds and the plain modes, an environment switch, launch counts, conditioned networks, one training step as a dict of
tensors, and the comparisons that more than one file makes.  Only what two files use is here; a file's own driver
(tests/test_gpu_half.py::_run and its like) stays with it.  Nothing here is rewritten by pytest, so every assert carries its
message."""
import os
import time

import torch

from oracle import wavenet_oracle as O
from tests import exactref as X
from tests.gpu_util import DEV

TOL = 1e-4                  # the project's bound on the fp32 and f16x3 paths, relative in max-norm
PLAIN = ("f16", "bf16")
UNFUSED = {"head": {"WN_SERIES_HEAD": "0"}, "entry": {"WN_SERIES_FRONT": "0"}, "both": {"WN_SERIES_HEAD": "0", "WN_SERIES_FRONT": "0"}}


class Env(object):
    """os.environ with `env` set inside the block, and put back after it"""

    def __init__(self, env):
        self.env, self.old = dict(env or {}), {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- launches ---------------------------------------------------------------------------------------------------------------------

def launched():
    """{kernel class: launches} of what the profile has counted"""
    from wavenet_speech_amd import functional as HF
    return {k: v[1] for k, v in HF.profile_read().items() if v[1]}


def launches(fn):
    """fn() with the launch profile on -> (what fn returned, {kernel class: launches})"""
    from wavenet_speech_amd import functional as HF
    HF.profile_reset()
    HF.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        HF.profile_enable(False)
    return out, launched()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    print("device part: %.3f s" % (time.time() - t0))
    return out


# ---- networks -----------------------------------------------------------------------------------------------------------------------

def condition(net, residual=True):
    """noisy biases and, unless residual=False, a conditioned residual path, as in a trained network"""
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape))
        blocks = list(net.convolutions) + ([net.input_block] if hasattr(net, "input_block") else [])
        for blk in blocks if residual else []:
            blk.residual_proj.weight.copy_(torch.eye(blk.out_channels, blk.in_channels)
                                           + 0.02 * torch.randn(blk.out_channels, blk.in_channels))
            blk.conv1x1_residual.weight.mul_(0.3)
    return net


def cycles_of(c, cycles):
    """(ci, co, k, d) of `cycles` times the dilations 1 .. 512 at c channels"""
    return [(c, c, 2, 2 ** i) for _ in range(cycles) for i in range(10)]


def wavenet(c, layers, seed=0, conditioned=True):
    """a seeded WaveNet on the CPU with noisy biases and, if conditioned, a residual path near the identity"""
    from wavenet_speech_amd.modules.wavenet import WaveNet
    torch.manual_seed(seed)
    return condition(WaveNet(c, 2, layers, c, softmax=False), residual=conditioned)


def onehot(b, c, l, seed):
    """(a one-hot input [b, c, l], a cotangent of the same shape), seeded"""
    g = torch.Generator().manual_seed(seed)
    return O.one_hot_encoding(torch.randint(0, c, (b, l), generator=g), c), torch.randn(b, c, l, generator=g)


def plain_slopes(net, xg):
    """the GPU's LeakyReLU pattern in a plain mode: one extra forward on the training path with the output block outside the stack
    function (as tests/test_gpu_half.py::_run takes it)"""
    slopes, handles = {}, []
    for name, mod in net.named_modules():
        if isinstance(mod, torch.nn.LeakyReLU):
            def hook(_m, inp, name=name, ns=mod.negative_slope):
                xin = inp[0].detach()
                slopes[name] = torch.where(xin > 0, torch.ones_like(xin), torch.full_like(xin, ns)).cpu()
            handles.append(mod.register_forward_pre_hook(hook))
    try:
        with Env({"WN_SERIES_HEAD": "0"}):
            net(xg.detach().requires_grad_(xg.requires_grad))
    finally:
        for h in handles:
            h.remove()
    return slopes


# ---- one step, and steps in a row -----------------------------------------------------------------------------------------------------

def step(net, x, cot, levels=False, input_grad=False, env=None):
    """{"forward", parameter names, "dx0"} of one forward and backward"""
    net.zero_grad(set_to_none=True)
    xg = x if levels else x.detach().clone().requires_grad_(input_grad)
    with Env(env):
        y = net.forward_levels(xg) if levels else net(xg)
        (y * cot).sum().backward()
    out = {"forward": y.detach().clone()}
    out.update({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    if input_grad:
        out["dx0"] = xg.grad.clone()
    return out


def same_step(a, b):
    """two dicts of step() hold the same names and the same bits"""
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


def train(net, x, cot, steps, graphed, lr):
    """`steps` Adam steps on (net(x) * cot).sum(), eager or through GraphedStep (on its own copies of x and cot) -> (losses, the
    eager warm-up steps the graphed run took first)"""
    import wavenet_speech_amd as W
    from wavenet_speech_amd.parallel import FlatGradAllReduce
    opt = torch.optim.Adam(net.parameters(), lr=lr, fused=True, capturable=True)
    sync = FlatGradAllReduce(net.parameters())
    losses = []
    if graphed:
        xs, cs = x.clone(), cot.clone()
        g = W.GraphedStep(lambda: (net(xs) * cs).sum(), net.parameters(), optimizer=opt, sync=sync, warmup=2)
        for _ in range(steps):
            losses.append(float(g()))
        g.check()
        return losses, 2
    for _ in range(steps):
        sync.zero()
        loss = (net(x) * cot).sum()
        loss.backward()
        sync.reduce()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, 0


# ---- exact arithmetic (tests/exactref.py) -----------------------------------------------------------------------------------------------

def exact_dev(t, grad=False):
    """a tensor of an exact case on the device as fp32; it must be representable"""
    assert X.is_fp32(t), "a value of the case is no fp32 number"
    return t.float().to(DEV).requires_grad_(grad)


def exact_same(got, want, what):
    """every tensor of `want` is bit for bit in `got`; the message names the tensor and the first differing element"""
    missing = sorted(set(want) - set(got))
    assert not missing, (what, "missing", missing)
    for k in sorted(want):
        diff = X.first_difference(got[k], want[k].float())
        assert diff is None, "%s: %s differs, first at %s: got %r, exact %r (%s)" % ((what, k) + diff[:3] + (diff[3:],))


def assert_saved_gate(fn_node, want_sg, want_z, what):
    """the precondition of a case, on what the function saved for backward: sigmoid and z are the three-valued ones"""
    _x, sg, z = fn_node.saved[:3]
    exact_same({"sg": sg.view(), "z": z.view()}, {"sg": want_sg, "z": want_z}, what + " (precondition: saved gate)")


# ---- the golden vectors and the size-independent properties (tests/test_gpu_parity.py, test_gpu_fullsize.py, test_gpu_half.py) -----------

def compare_grads(g, module, tol=TOL):
    for k, p in module.named_parameters():
        if not g.hasgrad[k]:
            continue
        assert p.grad is not None, k
        err = O.rel_err(p.grad.cpu(), g.grads[k])
        assert err < tol, (g.name, k, err)


def run_golden(g, module, tol=TOL):
    """a golden fixture through `module` on the device: every output, every parameter gradient and dx within tol"""
    missing = module.load_state_dict(g.sd, strict=True)  # reference checkpoints must load unchanged
    assert not missing.missing_keys and not missing.unexpected_keys, (g.name, missing)
    module = module.to(DEV)
    x = g.inputs["x"].to(DEV).requires_grad_(True)
    outs = module(x)
    if not isinstance(outs, tuple):
        outs = (outs,)
    assert len(outs) == len(g.outs), (g.name, len(outs), len(g.outs))
    loss = 0
    for o, ref, cot in zip(outs, g.outs, g.cots):
        assert tuple(o.shape) == tuple(ref.shape), (g.name, tuple(o.shape), tuple(ref.shape))
        err = O.rel_err(o.detach().cpu(), ref)
        assert err < tol, (g.name, "forward", err)
        loss = loss + (o * cot.to(DEV)).sum()
    loss.backward()
    compare_grads(g, module, tol)
    err = O.rel_err(x.grad.cpu(), g.grad_inputs["x"])
    assert err < tol, (g.name, "dx", err)


def properties(net, x, cot, prefix, split, causal_prefix, additivity_tol=1e-5):
    """size-independent properties at a configuration's full size: bitwise determinism of outputs and gradients,
    [causality: prefix of the output == output of the prefix], batch additivity of the weight gradients,
    per-utterance independence."""
    def grads(xs, cs):
        net.zero_grad(set_to_none=True)
        y = net(xs)
        (y * cs).sum().backward()
        return y.detach(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    y, g_all = grads(x, cot)
    y2, g_again = grads(x, cot)
    assert torch.equal(y, y2) and all(torch.equal(g_all[k], g_again[k]) for k in g_all), "a rerun gave other bits"
    assert bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(v).all()) for v in g_all.values()), "a value that is not finite"
    if causal_prefix:
        y_prefix = net(x[:, :, :prefix].contiguous()).detach()     # same grad mode as y (see test_cfg3_full_batch_properties)
        assert torch.equal(y_prefix, y[:, :, :prefix]), "the output of the prefix is not the prefix of the output"
    _, g_a = grads(x[:split].contiguous(), cot[:split].contiguous())
    _, g_b = grads(x[split:].contiguous(), cot[split:].contiguous())
    for k in g_all:
        err = O.rel_err((g_a[k] + g_b[k]).cpu(), g_all[k].cpu())
        assert err < additivity_tol, (k, err)
    i = x.shape[0] - 1
    yi = net(x[i:i + 1].contiguous()).detach()
    assert torch.equal(yi[0], y[i]), "the last utterance alone gives other bits"
    return y
