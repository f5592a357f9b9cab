"""GPU: the fp32 conv, block, stack and whole step, and the f16x3 conv and stack, against the exact references of tests/exactref.py --
BITWISE.  The inputs lie on a dyadic grid on which no fp32 partial sum ever rounds (proved on the CPU by exactref.assert_exact
before the device is touched), so any tiling, summation order, split-K or accumulate pass must return the integer-arithmetic
result bit for bit: every comparison is torch.equal, and a single wrong element of any size fails -- a lost tap at a tile clip, a
wgrad slab that drops a 32-step chunk, a reduce that skips a slab, an f16x3 product without one of its cross terms.

Two points rest on the hardware: v_rcp_f32(2) = 0.5 and the saturation values of the exp2 / rcp tanh and sigmoid.
test_gate_values_at_multiples_of_q (and its f16x3 twin) asserts them on their own; every fp32 block and stack test asserts them
on the saved sigmoid / z of its own case before it looks at anything else."""
import time

import pytest
import torch

from wavenet_speech_amd import _lib
from wavenet_speech_amd import functional as HF
from wavenet_speech_amd import functional_half as HH
from wavenet_speech_amd.modules.block import ResidualBlock, fusable_head, run_stack
from wavenet_speech_amd.modules.wavenet import WaveNet

from tests import exactref as X
from tests.gpu_stack import UNFUSED, Env as _Env, assert_saved_gate as _assert_saved_gate, exact_dev as _dev, exact_same as _same
from tests.gpu_stack import launches as _launches, timed as _timed
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------
# the preconditions on the card
# ------------------------------------------------------------------------------------------------------------------
def test_gate_values_at_multiples_of_q():
    """tanh(Q m) in {-1, 0, 1} and sigmoid(Q n) in {0, 1/2, 1} exactly, read as z = tanh sigmoid through an identity skip
    projection: a = x (identity on the last tap), g = its channel's bias"""
    c, L = 32, 7
    blk = ResidualBlock(c, c, 2, 1).to(DEV)
    ms = torch.tensor([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 5.0])
    ns = torch.tensor([(-1.0, 0.0, 1.0, -4.0, 3.0)[i % 5] for i in range(c)])
    with torch.no_grad():
        for p in blk.parameters():
            p.zero_()
        blk.conv_tanh.conv1d.weight[:, :, 1] = torch.eye(c)
        blk.conv_sigmoid.conv1d.bias.copy_(ns * X.Q)
        blk.conv1x1_skip.weight[:, :, 0] = torch.eye(c)
        x = (ms * X.Q).view(1, 1, L).expand(1, c, L).contiguous()
        _, z = blk(x.to(DEV))
    ta, sg = X.gate3(x.double(), (ns.double() * X.Q).view(1, c, 1).expand(1, c, L))
    seen = sorted(set(z.cpu().flatten().tolist()))
    print("z values at multiples of %g: %s" % (X.Q, seen))
    assert X.pairs_seen(ta, sg) == set(X.NINE)
    _same({"z": z}, {"z": ta * sg}, "gate")
    assert seen == [-1.0, -0.5, 0.0, 0.5, 1.0]


# ------------------------------------------------------------------------------------------------------------------
# a. fp32 conv
# ------------------------------------------------------------------------------------------------------------------
def _run_conv(c, precision):
    x, w, dy = _dev(c.x, True), _dev(c.w, True), _dev(c.dy)
    b = _dev(c.b, True) if c.b is not None else None
    y = HF.dilated_conv(x, w, b, c.d, c.causal, precision)
    y.backward(dy)
    with torch.no_grad():
        y_inf = HF.dilated_conv(x, w, b, c.d, c.causal, precision)
    got = {"y": y.detach(), "dx": x.grad, "dw": w.grad, "y (no_grad)": y_inf}
    if b is not None:
        got["db"] = b.grad
    return got


@pytest.mark.parametrize("case", X.CONV_CASES + ["no_bias"])
def test_f32_conv_is_exact(case):
    c = X.conv_case(X.CONV_NO_BIAS, False) if case == "no_bias" else X.conv_case(case)
    X.assert_exact(c)
    got = _timed(lambda: _run_conv(c, "f32"))
    want = dict(c.ref)
    want["y (no_grad)"] = c.ref["y"]
    _same(got, want, "conv %s" % (case,))
    assert ("db" in got) == (c.b is not None)


# ------------------------------------------------------------------------------------------------------------------
# b. f16x3 conv
# ------------------------------------------------------------------------------------------------------------------
def test_f16x3_scales_are_the_emulated_ones():
    assert float(_lib.load().wn_hseries_residual_scale()) == X.RS and HH.GRAD_TARGET == X.GRAD_TARGET
    for amax in (3.0, 0.75, 4095.0 * 2.0 ** -10, 8191.0 * 2.0 ** -10):
        t = torch.zeros(64, device=DEV)
        t[5] = -amax
        s, inv = HH._grad_scale(t, HH._Mode("f16x3"))
        assert float(s) == X.grad_scale(t.cpu().double()) and float(inv) * float(s) == 1.0, (amax, float(s))


@pytest.mark.parametrize("cls", X.HALF_CLASSES)
@pytest.mark.parametrize("case", X.HALF_CONV_CASES)
def test_f16x3_conv_is_exact(case, cls):
    """class "none": both low planes are zero (tiling and layout); "x" / "w" / "dy": that operand needs both planes and meets
    few-bit partners, so a dropped cross product changes the result"""
    c = X.half_conv_case(case, cls)
    X.assert_exact(c)
    got = _timed(lambda: _run_conv(c, "f16x3"))
    HH.check_fp16_overflow()
    want = dict(c.ref)
    want["y (no_grad)"] = c.ref["y"]
    _same(got, want, "f16x3 conv %s, two planes: %s" % (case, cls))


# ------------------------------------------------------------------------------------------------------------------
# c. fp32 block
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", X.GATE_MODES)
@pytest.mark.parametrize("case", X.BLOCK_CASES)
def test_f32_block_is_exact(case, mode):
    ci, co, k, d, causal, L, Bn = case
    c = X.block_case(case, mode)
    X.assert_exact(c)
    if mode == "mixed":
        # (B L = 1 has eight gate elements: eight of the nine pairs)
        assert len(c.pairs) >= c.want_pairs and c.want_pairs == min(9, Bn * L * co), sorted(c.pairs)
    blk = ResidualBlock(ci, co, k, d, causal=causal)
    blk.load_state_dict({k_: v.float() for k_, v in c.p.items()})
    blk = blk.to(DEV)
    x = _dev(c.x, True)

    def run():
        r, s = blk(x)
        _assert_saved_gate(r.grad_fn, c.ref["sg"], c.ref["z"], "block %s %s" % (case, mode))
        torch.autograd.backward([r, s], [_dev(c.dr), _dev(c.ds)])
        with torch.no_grad():
            r2, s2 = blk(x)
        return r.detach(), s.detach(), r2, s2
    r, s, r2, s2 = _timed(run)
    got = {"r": r, "s": s, "dx": x.grad, "r (no_grad)": r2, "s (no_grad)": s2}
    got.update({k_: p.grad for k_, p in blk.named_parameters()})
    want = {k_: v for k_, v in c.ref.items() if k_ not in ("sg", "z", "da", "dg")}
    want.update({"r (no_grad)": c.ref["r"], "s (no_grad)": c.ref["s"]})
    assert len(want) == 15
    _same(got, want, "block %s %s" % (case, mode))


# ------------------------------------------------------------------------------------------------------------------
# d. fp32 stack and whole step
# ------------------------------------------------------------------------------------------------------------------
def _net(c):
    net = WaveNet(X.IN, 2, c.layers, X.MS, softmax=False)
    net.output_stack[0].negative_slope, net.output_stack[2].negative_slope = X.SLOPES
    missing, unexpected = net.load_state_dict({k: v.float() for k, v in c.sd.items()}, strict=False)
    assert not unexpected and (c.kind == "net") == (not missing), (missing, unexpected)
    return net.to(DEV)


def _assert_saved_gates_of_stack(node, c, what):
    n = len(c.layers)
    assert len(node.saved) == n
    for l, (name, a, g) in enumerate(c.gates):
        ta, sg = X.gate3(a, g)
        _x, dsg, dz = node.saved[l][:3]
        _same({"sg": dsg.view(), "z": dz.view()}, {"sg": sg, "z": ta * sg}, "%s block %d (precondition: saved gate)" % (what, l))


@pytest.mark.parametrize("L", X.LENGTHS)
@pytest.mark.parametrize("stack", sorted(X.STACKS))
def test_f32_stack_is_exact(stack, L):
    c = X.stack_case(stack, L)
    X.assert_exact(c)
    assert len(c.pairs) == 9
    net = _net(c)
    x = _dev(c.x, True)
    what = "stack %s L=%d" % (stack, L)

    def run():
        S = run_stack(x, net.convolutions, net.bottlenecks, net.stack_state)
        _assert_saved_gates_of_stack(S.grad_fn, c, what)
        S.backward(_dev(c.cot))
        with torch.no_grad():
            S2 = run_stack(x, net.convolutions, net.bottlenecks, net.stack_state)
        return S.detach(), S2
    S, S2 = _timed(run)
    got = {"forward": S, "forward (no_grad)": S2, "dx0": x.grad}
    got.update({k: p.grad for k, p in net.named_parameters() if p.grad is not None})
    want = {k: v for k, v in c.ref.items() if not k.startswith("block") and k != "skips_sum"}
    want["forward (no_grad)"] = c.ref["forward"]
    _same(got, want, what)
    # the residual output of the last block is unused: no gradient at all for its conv1x1_residual and residual_proj
    assert set(got) == set(want), sorted(set(got) ^ set(want))


# ------------------------------------------------------------------------------------------------------------------
# e. f16x3 stack
# ------------------------------------------------------------------------------------------------------------------
def test_f16x3_gate_values_at_multiples_of_q():
    """the half path's h_tanh / h_sigmoid at multiples of Q, read as skips_sum = z through an identity skip projection and an
    identity bottleneck (inference: the per-block form)"""
    import torch.nn as nn
    from wavenet_speech_amd.modules.block import StackState
    c, L = 32, 7
    blk, bott, state = ResidualBlock(c, c, 2, 1).to(DEV), nn.Conv1d(c, c, 1).to(DEV), StackState()
    state.precision = "f16x3"
    ms = torch.tensor([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 5.0])
    ns = torch.tensor([(-1.0, 0.0, 1.0, -4.0, 3.0)[i % 5] for i in range(c)])
    with torch.no_grad():
        for p in list(blk.parameters()) + list(bott.parameters()):
            p.zero_()
        blk.conv_tanh.conv1d.weight[:, :, 1] = torch.eye(c)
        blk.conv_sigmoid.conv1d.bias.copy_(ns * X.Q)
        blk.conv1x1_skip.weight[:, :, 0] = torch.eye(c)
        bott.weight[:, :, 0] = torch.eye(c)
        x = (ms * X.Q).view(1, 1, L).expand(1, c, L).contiguous()
        z = run_stack(x.to(DEV), [blk], [bott], state)
    HH.check_fp16_overflow()
    ta, sg = X.gate3(x.double(), (ns.double() * X.Q).view(1, c, 1).expand(1, c, L))
    print("f16x3 z values at multiples of %g: %s" % (X.Q, sorted(set(z.cpu().flatten().tolist()))))
    _same({"z": z}, {"z": ta * sg}, "f16x3 gate")


def test_f16x3_stack_is_exact():
    """the three_k2 stack at L = 130 through set_precision(net, "f16x3"), on the grid that exactref's plane-by-plane emulation
    proves exact (tests/test_exactref.py::test_f16x3_stack_grid_is_exact)"""
    import wavenet_speech_amd as W
    c = X.stack_case("three_k2", 130, False, True)
    X.assert_exact(c)
    assert len(c.pairs) == 9 and c.products.hscale
    net = W.set_precision(_net(c), "f16x3")
    x = _dev(c.x, True)

    def run():
        S = run_stack(x, net.convolutions, net.bottlenecks, net.stack_state)
        S.backward(_dev(c.cot))
        with torch.no_grad():
            S2 = run_stack(x, net.convolutions, net.bottlenecks, net.stack_state)
        return S.detach(), S2
    (S, S2), ran = _launches(lambda: _timed(run))
    HH.check_fp16_overflow()
    assert any(k.startswith("h") for k in ran) and not any(k.startswith("series_gemm_kernel") for k in ran), ran
    got = {"forward": S, "forward (no_grad)": S2, "dx0": x.grad}
    got.update({k: p.grad for k, p in net.named_parameters() if p.grad is not None})
    want = {k: v for k, v in c.ref.items() if not k.startswith("block") and k != "skips_sum"}
    want["forward (no_grad)"] = c.ref["forward"]
    _same(got, want, "f16x3 stack")
    assert set(got) == set(want), sorted(set(got) ^ set(want))


def _step(net, c, levels=False, input_grad=False, env=None, check_gates=None):
    net.zero_grad(set_to_none=True)
    xg = c.levels.to(DEV) if levels else _dev(c.x, input_grad)
    with _Env(env):
        y = net.forward_levels(xg) if levels else net(xg)
        if check_gates:
            _assert_saved_gates_of_stack(y.grad_fn, c, check_gates)
        y.backward(_dev(c.cot))
    out = {"forward": y.detach().clone()}
    out.update({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    if input_grad:
        out["dx0"] = xg.grad.clone()
    return out


@pytest.mark.parametrize("stack,L", X.NET_CASES)
def test_f32_training_step_is_exact(stack, L):
    """entry conv, stack, folded bottlenecks, the long-K skips_sum, the fused LeakyReLU head, every parameter gradient and the
    input gradient; through forward (input gradient wanted or not), forward_levels, the op-by-op forms and under no_grad, whose
    block-by-block skips_sum must equal the long-K one here.  Row ZERO_ROW of skips_sum is exactly 0 and takes the slope."""
    c = X.stack_case(stack, L, net=True)
    X.assert_exact(c)
    assert len(c.pairs) == 9 and c.zero_row_is_zero
    net = _net(c)
    n = len(c.layers)
    what = "net %s L=%d" % (stack, L)
    assert fusable_head(net.output_stack, "f32") is not None
    want = {k: v for k, v in c.ref.items() if not k.startswith("block") and k != "skips_sum"}
    no_dx0 = {k: v for k, v in want.items() if k != "dx0"}
    t0 = time.time()
    fused, ran = _launches(lambda: _step(net, c, input_grad=True, check_gates=what))
    _same(fused, want, what + " forward, input gradient")
    assert set(fused) == set(want), sorted(set(fused) ^ set(want))
    # the launch classes the case exists for
    assert ran["pack_kernel"] == 1, ran
    assert ran["series_gemm_kernel<skips_sum>"] == 1 and ran["series_gemm_kernel<gate>"] == n, ran
    assert ran["series_gemm_kernel<conv_fwd>"] == 3 and ran["series_gemm_kernel<conv_bwd_data>"] == 3, ran
    assert ran["wgrad_kernel"] >= n + 3 and ran["wgrad_reduce_kernel"] >= 1, ran
    plain = _step(net, c)
    _same(plain, no_dx0, what + " forward")
    assert "dx0" not in plain
    _same(_step(net, c, levels=True), no_dx0, what + " forward_levels")
    for name, env in sorted(UNFUSED.items()):
        _same(_step(net, c, input_grad=True, env=env), want, what + " op by op: " + name)
        _same(_step(net, c, levels=True, env=env), no_dx0, what + " forward_levels, op by op: " + name)
    with torch.no_grad():
        y = net(_dev(c.x))
        yl = net.forward_levels(c.levels.to(DEV))
        with _Env(UNFUSED["both"]):
            y0 = net(_dev(c.x))
    _same({"forward": y}, {"forward": c.ref["forward"]}, what + " no_grad")
    _same({"forward": yl}, {"forward": c.ref["forward"]}, what + " no_grad, forward_levels")
    _same({"forward": y0}, {"forward": c.ref["forward"]}, what + " no_grad, op by op")
    torch.cuda.synchronize()
    print("device part: %.3f s" % (time.time() - t0))
