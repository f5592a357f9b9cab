"""GPU: the fp32 step with its entry conv and output block in the series layout (functional._ResidualStackFn with `front` / `head`)
against the op-by-op form it replaces -- BITWISE: the fused form changes no product's tiling, K order or rounding, and LeakyReLU
in the epilogues is torch's own rule -- and the op-by-op fallback against an fp64 reference.

Shapes are the smallest that reach the edges: 40 channels (a ragged 32-row tile, cp8 padding), skip / out dim 24, k = 2 blocks at
dilations 1, 2, 4 and a stack of one k = 3 block, B = 2, L in {130 (a full 128-column tile and a 2-column one: the clip), 128 (one
tile exactly), 5 (shorter than a dilation)}."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from wavenet_speech_amd.modules.block import fusable_head, run_stack
from wavenet_speech_amd.modules.pointwise import run_sequential
from wavenet_speech_amd.modules.wavenet import WaveNet

from oracle import wavenet_oracle as O
from tests.gpu_stack import TOL, UNFUSED, Env as _Env, launches as _launches, same_step as _same, step as _step, train as _train
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
C, MS, IN, B = 40, 24, 11, 2
STACKS = {"three_k2": [(C, C, 2, 1), (C, C, 2, 2), (C, C, 2, 4)], "one_k3": [(C, C, 3, 2)]}
LENGTHS = [130, 128, 5]


def _net(stack, seed):
    torch.manual_seed(seed)
    net = WaveNet(IN, 2, STACKS[stack], MS, softmax=False)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:                      # the reference's init zeroes every bias: give them values
                p.normal_(0.0, 0.1)
    return net.to(DEV)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_fused_step_is_bitwise_the_op_by_op_step(stack, L):
    """the output, every parameter gradient and the input gradient: the series head against head=None + run_sequential, the
    entry-conv hand-off against the dense hand-off, through forward (input gradient wanted or not) and forward_levels"""
    net = _net(stack, 11 + L)
    assert fusable_head(net.output_stack, "f32") is not None
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, IN, L, generator=g).to(DEV)
    q = torch.randint(0, IN, (B, L), generator=g).to(DEV)
    cot = torch.randn(B, MS, L, generator=g).to(DEV)
    for levels, input_grad in ((False, False), (False, True), (True, False)):
        inp = q if levels else x
        fused = _step(net, inp, cot, levels, input_grad)
        assert ("dx0" in fused) == input_grad
        for what, env in sorted(UNFUSED.items()):
            _same(fused, _step(net, inp, cot, levels, input_grad, env))
    # the fused step launches no stand-alone pack per block and one pack in all
    n = len(STACKS[stack])
    _, ran = _launches(lambda: _step(net, x, cot))
    assert ran["pack_kernel"] == 1, ran
    assert ran["series_gemm_kernel<conv_fwd>"] == 3 and ran["series_gemm_kernel<conv_bwd_data>"] == 2, ran
    assert ran["series_gemm_kernel<skips_sum>"] == 1 and ran["series_gemm_kernel<gate>"] == n, ran


@pytest.mark.parametrize("L", [130, 5])
def test_inference_is_bitwise_the_op_by_op_forward(L):
    net = _net("three_k2", 3)
    x = torch.randn(B, IN, L, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        y = net(x)
        with _Env(UNFUSED["both"]):
            y0 = net(x)
    assert torch.equal(y, y0)
    yt = net(x)                      # the training forward forms skips_sum by one long-K product, inference block by block
    assert O.rel_err(y.cpu(), yt.detach().cpu()) < 1e-5


def test_activation_of_exactly_zero_takes_the_slope():
    """torch's rule is x > 0 ? 1 : slope, so an element of skips_sum that is exactly 0 passes slope * gradient.  Row 7 of every
    bottleneck (weights and bias) is zeroed: row 7 of each folded skip projection and of the summed bias is then exactly 0, and so
    is that row of skips_sum."""
    row = 7
    net = _net("three_k2", 5)
    with torch.no_grad():
        for b in net.bottlenecks:
            b.weight[row].zero_()
            b.bias[row].zero_()
    L = 130
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, IN, L, generator=g).to(DEV)
    cot = torch.randn(B, MS, L, generator=g).to(DEV)
    with _Env(UNFUSED["both"]):
        S, done = run_stack(net.entry_conv1d(x), net.convolutions, net.bottlenecks, net.stack_state, head=net.output_stack)
    assert not done and float(S.detach()[:, row].abs().max()) == 0.0
    fused = _step(net, x, cot, input_grad=True)
    _same(fused, _step(net, x, cot, input_grad=True, env=UNFUSED["both"]))
    # the zero row carries slope * (W1^T dh)[row], not 0 and not the whole gradient: d loss / d bottleneck bias[row] is its sum
    for l in range(3):
        gb = fused["bottlenecks.%d.bias" % l]
        assert float(gb[row].abs()) > 0.0
    S = S.detach().requires_grad_(True)
    (run_sequential(net.output_stack[1:], F.leaky_relu(S, 0.01)) * cot).sum().backward()       # torch's own backward rule
    want = S.grad[:, row]
    assert float(want.abs().max()) > 0.0
    assert abs(float(fused["bottlenecks.2.bias"][row]) - float(want.sum())) <= 1e-5 * float(want.abs().sum())


def test_hooks_on_the_output_block_keep_it_op_by_op():
    """a fused block never calls its modules, so forward hooks on them would not run: the fp32 mode then evaluates the block op by
    op (bitwise the same result), through forward and forward_levels alike"""
    net = _net("three_k2", 13)
    L = 130
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, IN, L, generator=g).to(DEV)
    q = torch.randint(0, IN, (B, L), generator=g).to(DEV)
    cot = torch.randn(B, MS, L, generator=g).to(DEV)
    plain = [_step(net, x, cot), _step(net, q, cot, levels=True)]
    seen = []
    handle = net.output_stack[2].register_forward_pre_hook(lambda _m, inp: seen.append(tuple(inp[0].shape)))
    try:
        assert fusable_head(net.output_stack, "f32") is None
        hooked = [_step(net, x, cot), _step(net, q, cot, levels=True)]
    finally:
        handle.remove()
    assert seen == [(B, MS, L)] * 2
    assert fusable_head(net.output_stack, "f32") is not None
    for a, b in zip(plain, hooked):
        _same(a, b)


def _fp64_reference(net, sd, x, cot, slopes):
    """the model in fp64: the oracle's entry conv and stack, then the head as torch evaluates its own modules, with the captured
    LeakyReLU pattern"""
    sdl = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    layers = [(b.in_channels, b.out_channels, b.kernel_width, b.dilation) for b in net.convolutions]
    out = O.dilated_conv(xr, sdl["entry_conv1d.conv1d.weight"], sdl["entry_conv1d.conv1d.bias"], 1, True)
    skips = torch.zeros(x.shape[0], MS, x.shape[2], dtype=torch.float64)
    _, y = O.block_stack(out, skips, sdl, layers, True)
    for i, mod in enumerate(net.output_stack):
        if isinstance(mod, nn.LeakyReLU):
            y = y * slopes["output_stack.%d" % i].double()
        else:
            bias = sdl.get("output_stack.%d.bias" % i)
            y = F.conv1d(y, sdl["output_stack.%d.weight" % i], bias, padding=mod.padding[0])
    (y * cot.double()).sum().backward()
    want = {"forward": y.detach(), "dx0": xr.grad}
    want.update({k: v.grad for k, v in sdl.items() if v.grad is not None})
    return want


def _head(kind):
    if kind == "no_bias":
        return nn.Sequential(nn.LeakyReLU(0.01), nn.Conv1d(MS, MS, 1, bias=False), nn.LeakyReLU(0.01), nn.Conv1d(MS, MS, 1))
    if kind == "negative_slope":
        return nn.Sequential(nn.LeakyReLU(-0.2), nn.Conv1d(MS, MS, 1), nn.LeakyReLU(0.01), nn.Conv1d(MS, MS, 1))
    assert kind == "k3"
    return nn.Sequential(nn.LeakyReLU(0.01), nn.Conv1d(MS, MS, 3, padding=2), nn.LeakyReLU(0.01), nn.Conv1d(MS, MS, 1))


@pytest.mark.parametrize("kind", ["no_bias", "negative_slope", "k3"])
def test_heads_outside_the_pattern_run_op_by_op_and_match_fp64(kind):
    L = 130
    torch.manual_seed(21)
    net = WaveNet(IN, 2, STACKS["three_k2"], MS, softmax=False)
    net.output_stack = _head(kind)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.1)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.to(DEV)
    assert fusable_head(net.output_stack, "f32") is None
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, IN, L, generator=g)
    cot = torch.randn(B, MS, L + (2 if kind == "k3" else 0), generator=g)
    slopes, remove = O.capture_leaky_slopes(net)
    xg = x.to(DEV).requires_grad_(True)
    _, ran = _launches(lambda: (net(xg) * cot.to(DEV)).sum().backward())
    remove()
    assert set(slopes) == {"output_stack.0", "output_stack.2"}          # the LeakyReLU modules ran: the head was not fused
    # three convs forward in the measured pass (entry in the series, two of the head on their own) + three in the pattern pass
    assert ran["series_gemm_kernel<conv_fwd>"] == 6, ran
    net.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    y = net(xg)
    (y * cot.to(DEV)).sum().backward()
    got = {"forward": y.detach().cpu(), "dx0": xg.grad.cpu()}
    got.update({k: p.grad.cpu() for k, p in net.named_parameters() if p.grad is not None})
    want = _fp64_reference(net, sd, x, cot, slopes)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    errs = {k: O.rel_err(got[k].double(), want[k]) for k in want}
    worst = max(errs, key=errs.get)
    print("%s: worst %s %.2e" % (kind, worst, errs[worst]))
    assert errs[worst] < TOL, errs


def test_graphed_step_replays_bitwise_the_eager_steps():
    """a small fp32 WaveNet step captured by GraphedStep, replayed twice with a weight update between the replays, equals the eager
    steps.  The pack table is uploaded during the warm-up, outside the captured region; the one captured pack launch reads the
    weights the optimizer has just written, and the folded skip projections through their storages' addresses in the graph's pool."""
    import copy
    L = 130
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, IN, L, generator=g).to(DEV)
    cot = torch.randn(B, MS, L, generator=g).to(DEV)
    base = _net("three_k2", 9)
    nets = [copy.deepcopy(base), copy.deepcopy(base)]
    lg, warm = _train(nets[1], x, cot, 2, graphed=True, lr=1e-2)
    le, _ = _train(nets[0], x, cot, 2 + warm, graphed=False, lr=1e-2)     # the graphed run took `warm` eager steps before its capture
    assert lg == le[warm:], (lg, le)
    assert lg[0] != lg[1]                                        # the weights did move between the replays
    for (k, a), (_, b) in zip(nets[0].state_dict().items(), nets[1].state_dict().items()):
        assert torch.equal(a, b), k
