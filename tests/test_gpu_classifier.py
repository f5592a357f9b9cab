"""GPU: WaveNetClassifier -- AvgPool1d fused into the load of the stack's input (csrc/wn_front.hip), the non-causal stack, the
output block -- forward, dx and every parameter gradient, in all four precisions.

f32 and f16x3 are held to the project's 1e-4 against the oracle (oracle.wavenet_classifier).  The plain modes are held to the error
their storage format implies: tests/halfref.py::wavenet_classifier, predicate e_hip <= KAPPA e_fmt + FLOOR in max-norm and RMS.
References that pool differently -- each what a plausible kernel bug would compute -- must be REJECTED for the unaltered GPU result."""
import pytest
import torch

import wavenet_speech_amd as W
from oracle import wavenet_oracle as O
from tests import halfref as R
from tests.gpu_stack import PLAIN, TOL, Env as _Env, condition as _condition, launched as _launched, plain_slopes as _plain_slopes
from tests.gpu_util import DEV
from wavenet_speech_amd import functional as HF

pytestmark = pytest.mark.gpu
PRECISIONS = ("f32", "f16x3", "bf16", "f16")


def _classifier(in_dim, layers, out_dim, pool, kw=2, dil=1, seed=0):
    from wavenet_speech_amd.modules.classifier import WaveNetClassifier
    torch.manual_seed(seed)
    net = WaveNetClassifier(in_dim, 5, layers, out_dim, pool_kernel_size=pool, input_kernel_size=kw, input_dilation=dil, softmax=False)
    return _condition(net)


def gpu_run(net, x, cot, precision, input_grad=True, env=None):
    """(tensors {"forward", "dx0", parameter names}, LeakyReLU slopes, launched kernels) of one forward and backward on the GPU"""
    net = net.to(DEV)
    W.set_precision(net, precision)
    xg = x.to(DEV).requires_grad_(input_grad)
    with _Env(env):
        if precision in PLAIN:
            slopes, remove = _plain_slopes(net, xg), lambda: None
        else:
            slopes, remove = O.capture_leaky_slopes(net)
        net.zero_grad(set_to_none=True)
        HF.profile_reset()
        HF.profile_enable(True)
        try:
            y = net(xg)
            remove()
            (y * cot.to(DEV)).sum().backward()
            torch.cuda.synchronize()
        finally:
            HF.profile_enable(False)
    W.check_device_flags()
    hip = {"forward": y.detach().cpu()}
    if input_grad:
        hip["dx0"] = xg.grad.cpu()
    hip.update({k: p.grad.cpu() for k, p in net.named_parameters() if p.grad is not None})
    return hip, slopes, _launched()


def reference(net, sd, x, cot, layers, pool, precision, slopes, input_grad, fmt, pool_mutant=None):
    """{name: tensor} of tests/halfref.py::wavenet_classifier in fp64 (fmt None: exact) as `net` runs in `precision`"""
    from wavenet_speech_amd.modules.block import fusable_head
    fused = fusable_head(net.output_block, precision) is not None
    ib = net.input_block

    def fn(xx, s, f):
        return R.wavenet_classifier(xx, s, layers, pool, f, input_dilation=ib.dilation, input_kwidth=ib.kernel_width, slopes=slopes,
                                    fused=fused, pool_mutant=pool_mutant)
    y, g = R.run(fn, [x.clone().requires_grad_(input_grad)], sd, cot, fmt)
    g["forward"] = y
    return g


def check_classifier(net, x, cot, layers, pool, precision, input_grad=True, kernels=None, mutants=(), label="", env=None):
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    hip, slopes, launched = gpu_run(net, x, cot, precision, input_grad, env)
    if kernels is not None:
        assert kernels(launched), launched
    tag = "%s%s" % (precision, label)
    if precision in PLAIN:
        exact = reference(net, sd, x, cot, layers, pool, precision, slopes, input_grad, None)
        assert set(exact) == set(hip), sorted(set(exact) ^ set(hip))
        rounded = reference(net, sd, x, cot, layers, pool, precision, slopes, input_grad, precision)
        out = R.check(tag, hip, rounded, exact)
        for m in mutants:
            e2 = reference(net, sd, x, cot, layers, pool, precision, slopes, input_grad, None, m)
            r2 = reference(net, sd, x, cot, layers, pool, precision, slopes, input_grad, precision, m)
            got = R.compare("%s mutant %s" % (tag, m), hip, r2, e2, quiet=True)
            bad = sorted(k for k, v in got.items() if not v[2])
            print("%s mutant %s: rejected by %d of %d tensors, e.g. %s" % (tag, m, len(bad), len(got), bad[:3]))
            assert bad, "mutant %s passes the predicate" % m
        return out, launched
    sdl = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(input_grad)
    y0 = O.wavenet_classifier(xr, sdl, layers, pool, net.input_block.dilation, False, slopes=slopes)
    (y0 * cot).sum().backward()
    want = {"forward": y0.detach()}
    if input_grad:
        want["dx0"] = xr.grad
    want.update({k: v.grad for k, v in sdl.items() if v.grad is not None})
    assert set(want) == set(hip), sorted(set(want) ^ set(hip))
    errs = {k: O.rel_err(hip[k], want[k]) for k in want}
    worst = max(errs, key=errs.get)
    print("%s: forward %.2e, dx %.2e, worst %s %.2e" % (tag, errs["forward"], errs.get("dx0", 0.0), worst, errs[worst]))
    assert errs[worst] < TOL, (worst, errs[worst])
    for m in mutants:
        e2 = reference(net, sd, x, cot, layers, pool, precision, slopes, input_grad, None, m)
        bad = sorted(k for k in want if not O.rel_err(hip[k].double(), e2[k]) < TOL)
        print("%s mutant %s: rejected by %d of %d tensors, e.g. %s" % (tag, m, len(bad), len(want), bad[:3]))
        assert bad, "mutant %s passes at %g" % (m, TOL)
    return errs, launched


def _ran(precision, input_grad, pool):
    """the kernels a case exists for: the stack's, and the pooled load / unload (profiled in the layout-load class hload_kernel)"""
    def ok(k):
        if precision == "f32":          # (the plain fp32 load is a torch copy: no kernel of this class without pooling)
            loads = k.get("hload_kernel", 0) >= 1 + int(input_grad) if pool > 1 else k.get("hload_kernel", 0) == 0
            return loads and k.get("series_gemm_kernel<gate>", 0) > 0 and k.get("wgrad_kernel", 0) > 0
        return k.get("hload_kernel", 0) >= 1 + int(input_grad and pool > 1) and "hwgrad_kernel" in k \
            and (k.get("hgemm_kernel<gate>", 0) > 0 or k.get("hfused_fwd_kernel", 0) > 0)
    return ok


CASES = {  # in_dim, layers, out_dim, pool, L, B, input kernel width, input dilation, input gradient
    # the plain load; in_dim not a multiple of 8; L one past a 128-column tile
    "pool1_in5": (5, [(16, 16, 2, 1), (16, 16, 3, 2)], 16, 1, 129, 3, 2, 1, True),
    # L // pool = 257 (one past a 256-column tile of the half layout, and 257 % 128 == 1), a tail of 1
    "pool2_in12_tail1": (12, [(32, 32, 2, 1), (32, 32, 2, 2)], 32, 2, 515, 1, 2, 1, True),
    # ONE pooled step, a tail of pool - 1; one past 32 input channels; k = 3 everywhere
    "pool3_in33_one_step": (33, [(32, 32, 3, 1), (32, 32, 3, 2)], 32, 3, 5, 3, 3, 1, True),
    # L // pool = 129, a tail of pool - 1; k = 3 blocks of changing width
    "pool5_in12_k3_tail4": (12, [(24, 24, 3, 1), (24, 40, 3, 2), (40, 40, 3, 5)], 24, 5, 649, 3, 2, 2, True),
    # L % pool = 0 at L // pool = 257
    "pool8_in33_exact": (33, [(64, 64, 2, d) for d in (1, 2, 4)], 64, 8, 2056, 1, 2, 1, True),
    "pool8_in5_tail7": (5, [(16, 16, 2, 1), (16, 32, 3, 3)], 16, 8, 327, 1, 3, 1, True),
    # the reference test's own width (tests/test_classifier.py: 256-dim in, 256-channel blocks, pool 3)
    "reference_width_256": (256, [(256, 256, 2, d) for d in (1, 2, 4)], 256, 3, 1500, 2, 2, 1, True),
    # data without gradient: no pool_unload launch, the bottom block's dx is not formed
    "pool3_no_input_grad": (12, [(32, 32, 2, 1), (32, 32, 2, 2)], 32, 3, 301, 3, 2, 1, False),
}


def _case(name):
    in_dim, layers, out_dim, pool, L, B, kw, dil, input_grad = CASES[name]
    net = _classifier(in_dim, layers, out_dim, pool, kw, dil, seed=len(name) + L)
    g = torch.Generator().manual_seed(L + B)
    x, cot = torch.randn(B, in_dim, L, generator=g), torch.randn(B, 5, L // pool, generator=g)
    return net, x, cot, layers, pool, input_grad


def test_cases_cover_the_edges():
    """the shapes above cover what the pooled classifier can get wrong (a list kept honest by a check, not by a comment)"""
    c = list(CASES.values())
    assert {v[3] for v in c} == {1, 2, 3, 5, 8}
    for pool in (2, 3, 5, 8):
        assert {0, pool - 1} & {v[4] % pool for v in c if v[3] == pool}
    assert any(v[4] % v[3] == 1 and v[3] > 2 or (v[3] == 2 and v[4] % 2 == 1) for v in c)
    assert {1, 257} <= {v[4] // v[3] for v in c} and any((v[4] // v[3]) % 128 == 1 for v in c)
    assert {v[0] for v in c} == {5, 12, 33, 256} and any(v[0] != v[1][0][0] for v in c)
    assert {1, 3} <= {v[5] for v in c} and any(l[2] == 3 for v in c for l in v[1]) and any(not v[8] for v in c)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_classifier_vs_reference(case, precision):
    net, x, cot, layers, pool, input_grad = _case(case)
    check_classifier(net, x, cot, layers, pool, precision, input_grad, kernels=_ran(precision, input_grad, pool), label=" " + case)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("case", ["pool5_in12_k3_tail4", "pool8_in5_tail7"])
def test_references_that_pool_differently_are_rejected(case, precision):
    """only the reference side changes: a window of pool + 1, a divisor of pool - 1, a window start one sample late, the tail folded
    into the last window, an input gradient not divided by pool"""
    net, x, cot, layers, pool, input_grad = _case(case)
    check_classifier(net, x, cot, layers, pool, precision, input_grad, mutants=R.POOL_MUTANTS, label=" " + case)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sequence_shorter_than_the_window_is_an_error(precision):
    net = _classifier(12, [(16, 16, 2, 1)], 16, 5, seed=1).to(DEV)
    W.set_precision(net, precision)
    x = torch.randn(2, 12, 4, device=DEV)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="shorter than the pooling window"):
            net(x)
    with pytest.raises(RuntimeError, match="shorter than the pooling window"):
        net(x.requires_grad_(True))
    with pytest.raises(RuntimeError, match="shorter than the pooling window"):
        net(x.detach())                                  # parameters alone need gradients: still the training path
    y = net(torch.randn(2, 12, 5, device=DEV))           # exactly one window is fine
    assert tuple(y.shape) == (2, 5, 1)
    W.check_device_flags()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ["pool5_in12_k3_tail4", "pool3_no_input_grad"])
def test_unfused_pooling_takes_the_torch_op_and_passes_the_same_bars(case, precision):
    """WN_POOL_FUSED=0: torch's avg_pool1d, then the plain load.  Each form is held to its reference on its own (the two half forms
    are not compared with each other); in f32 the two differ by the pooled load's own rounding (pool 2^-24 mean|x| per element,
    tests/test_pool.py), which the stack carries to the outputs like any fp32 input perturbation: both within 1e-4 of the oracle,
    and of each other."""
    net, x, cot, layers, pool, input_grad = _case(case)
    import copy
    _, fused = check_classifier(copy.deepcopy(net), x, cot, layers, pool, precision, input_grad, label=" fused " + case)
    _, unfused = check_classifier(copy.deepcopy(net), x, cot, layers, pool, precision, input_grad, label=" unfused " + case,
                                  env={"WN_POOL_FUSED": "0"})
    # the fused form replaces the plain load by the pooled one and adds the unload of the input gradient.  In f32 the plain load is a
    # torch copy, so both pooled loads count -- the measured forward's and that of the pattern-capturing forward, which
    # oracle.capture_leaky_slopes runs inside the profiled region
    assert fused.get("hload_kernel", 0) == unfused.get("hload_kernel", 0) + int(input_grad) + (2 if precision == "f32" else 0), \
        (fused, unfused)
    if precision == "f32":
        a, _, _ = gpu_run(copy.deepcopy(net), x, cot, precision, input_grad)
        b, _, _ = gpu_run(copy.deepcopy(net), x, cot, precision, input_grad, env={"WN_POOL_FUSED": "0"})
        errs = {k: O.rel_err(a[k], b[k]) for k in b}
        worst = max(errs, key=errs.get)
        print("f32 fused vs unfused pooling %s: worst %s %.2e" % (case, worst, errs[worst]))
        assert set(a) == set(b) and errs[worst] < TOL
