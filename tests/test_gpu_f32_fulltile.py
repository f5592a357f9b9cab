"""GPU: the full-tile form of the fp32 series GEMM's batched epilogues (EPI_DGATE, EPI_DMASK, EPI_ACCUM in csrc/wn_gemm.hip).

A wave whose 32 MT rows all lie below the destination's row count and whose 128 columns all lie below L runs a straight-line
copy of its epilogue; every other wave runs the ragged form.  Every other exact case of the suite has channels that are no
multiple of 64 or L < 128, so none reaches the full form: these do.

* the block cases of tests/test_gpu_exact.py::test_f32_block_is_exact restated at shapes with interior tiles, against the
  integer-arithmetic references of tests/exactref.py -- bit for bit;
* one stack through both forms: L = 128 with the cotangent zero from column 100 on, and L = 100 on the first 100 columns;
* EPI_DMASK and EPI_ACCUM at 64 rows and L = 128: the fused step against the op-by-op step, bit for bit, and the block-by-block
  skips_sum of inference against the one long-K product of the training forward."""
import pytest
import torch

from wavenet_speech_amd import functional as HF
from wavenet_speech_amd.modules.block import ResidualBlock, fold_bottlenecks, fusable_head, run_stack
from wavenet_speech_amd.modules.wavenet import WaveNet

from tests import exactref as X
from tests.gpu_stack import UNFUSED, assert_saved_gate as _assert_saved_gate, exact_dev as _dev, exact_same as _same
from tests.gpu_stack import launches as _launches, same_step as _same_bits, step as _step, timed as _timed
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


# (ci, co, k, d, causal, L, B); dz runs 64-row slabs (MT = 2) from 64 channels on, 128 columns per tile
FULL_TILE_CASES = [
    (64, 64, 2, 1, True, 128, 2),       # one slab, one tile, all interior, two utterances
    (64, 128, 2, 4, True, 256, 1),      # two slabs x two tiles, all interior
    (64, 96, 2, 2, True, 160, 2),       # interior and ragged rows x interior and ragged columns in one launch
    (128, 128, 2, 64, True, 128, 1),    # dilation beyond half the tile
]


@pytest.mark.parametrize("mode", X.GATE_MODES)
@pytest.mark.parametrize("case", FULL_TILE_CASES)
def test_f32_block_with_interior_tiles_is_exact(case, mode):
    ci, co, k, d, causal, L, Bn = case
    c = X.block_case(case, mode)
    X.assert_exact(c)
    if mode == "mixed":
        assert len(c.pairs) >= c.want_pairs and c.want_pairs == 9, sorted(c.pairs)
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


def test_full_and_ragged_forms_agree_on_the_first_100_columns():
    """a two-block causal stack at 64 channels.  At L = 128 every dz tile is interior; at L = 100 every one is ragged.  The model
    is causal and dz is pointwise in time, so with the cotangent zero from column 100 on, the outputs and the input gradient on
    the first 100 columns are the same bits (the columns beyond add exact zeros).  The last block has no residual gradient: its
    dz has one K segment.  Weight gradients are not compared: their split-K partition depends on L."""
    C, B, L, CUT = 64, 2, 128, 100
    torch.manual_seed(5)
    blocks = torch.nn.ModuleList([ResidualBlock(C, C, 2, 1), ResidualBlock(C, C, 2, 2)])
    with torch.no_grad():
        for p in blocks.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.1)
    blocks = blocks.to(DEV)
    specs = [b.spec() for b in blocks]
    flat = [p for b in blocks for p in b.hip_params()]
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, C, L, generator=g).to(DEV)
    cot = torch.randn(B, C, L, generator=g).to(DEV)
    cot[:, :, CUT:] = 0.0

    def run(n):
        xg = x[:, :, :n].contiguous().requires_grad_(True)
        S = HF.residual_stack(xg, specs, flat)
        S.backward(cot[:, :, :n].contiguous())
        return S.detach()[:, :, :CUT].clone(), xg.grad[:, :, :CUT].clone()
    S_full, dx_full = run(L)
    S_ragged, dx_ragged = run(CUT)
    assert float(dx_full.abs().max()) > 0.0
    assert torch.equal(S_full, S_ragged)
    assert torch.equal(dx_full, dx_ragged), float((dx_full - dx_ragged).abs().max())


C, MS, IN, B, L = 64, 64, 11, 2, 128
LAYERS = [(C, C, 2, 1), (C, C, 2, 2)]


def _net(seed):
    torch.manual_seed(seed)
    net = WaveNet(IN, 2, LAYERS, MS, softmax=False)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:                      # the reference's init zeroes every bias: give them values
                p.normal_(0.0, 0.1)
    return net.to(DEV)


def test_fused_step_on_full_tiles_is_bitwise_the_op_by_op_step():
    """EPI_DMASK: the head's backward-data product masks by the stored activation in its epilogue; op by op, torch's
    leaky_relu_backward does.  64 rows and L = 128: every tile of it is interior."""
    net = _net(31)
    assert fusable_head(net.output_stack, "f32") is not None
    g = torch.Generator().manual_seed(32)
    x = torch.randn(B, IN, L, generator=g).to(DEV)
    cot = torch.randn(B, MS, L, generator=g).to(DEV)
    fused = _step(net, x, cot, input_grad=True)
    for _what, env in sorted(UNFUSED.items()):
        _same_bits(fused, _step(net, x, cot, input_grad=True, env=env))
    _, ran = _launches(lambda: _step(net, x, cot))
    assert ran["series_gemm_kernel<conv_bwd_data>"] == 2 and ran["series_gemm_kernel<skips_sum>"] == 1, ran


def test_inference_accumulates_skips_on_full_tiles():
    """EPI_ACCUM: under no_grad skips_sum is accumulated block by block (a read-modify-write epilogue from the second block on);
    the training forward forms it by one long-K product.  Both are fp32 sums of the same K = 2 x 64 products and three biases in
    different orders.  Any order of n additions is within (n - 1) u sum |terms| of the exact sum to first order (u = 2^-24), so two
    orders differ by at most 2 (K + 2) u sum |terms|: asserted element by element, with sum |terms| = sum_l |W_l| |z_l| + |b_l|
    evaluated in fp64 from the z the training forward saved."""
    net = _net(33)
    x = torch.randn(B, C, L, generator=torch.Generator().manual_seed(34)).to(DEV)
    S = run_stack(x, net.convolutions, net.bottlenecks, net.stack_state)
    out = {}
    with torch.no_grad():
        _, ran = _launches(lambda: out.update(S=run_stack(x, net.convolutions, net.bottlenecks, net.stack_state)))
        wfs, bfs = fold_bottlenecks(list(net.convolutions), list(net.bottlenecks))
    S_inf = out["S"]
    assert ran["series_gemm_kernel<skips_sum>"] == len(LAYERS), ran
    terms = torch.zeros(B, MS, L, dtype=torch.float64, device=DEV)
    for l, (w, b) in enumerate(zip(wfs, bfs)):
        z = S.grad_fn.saved[l][2].view().double()
        terms += torch.einsum("oc,bcl->bol", w.double().abs(), z.abs()) + b.double().abs().view(1, MS, 1)
    K = sum(co for _ci, co, _k, _d in LAYERS)
    bound = 2.0 * (K + 2) * 2.0 ** -24 * terms
    diff = (S_inf.double() - S.detach().double()).abs()
    print("worst |difference| / bound: %.3f" % float((diff / bound).max()))
    assert bool((diff <= bound).all()), float((diff / bound).max())
