"""CPU: the exact path of the rounding reference (tests/halfref.py with fmt=None) is the oracle's model.  Every bound on the plain
half modes measures distances from it, so it is pinned here: forward and every gradient against oracle.wavenet / raw_ctcnet in
fp64.  Also: the rounding path differs from it by no more than its format."""
import pytest
import torch

from oracle import wavenet_oracle as O
from tests import halfref as R

LAYERS = [(16, 16, 2, 1), (16, 24, 3, 2), (24, 24, 2, 5), (24, 16, 3, 1)]


def _state(model, layers, kf=3, seed=0):
    if model == "wavenet":
        sd = O.random_wavenet_state(8, 2, layers, 12, seed=seed, dtype=torch.float64)
    else:
        sd = O.random_rawctcnet_state(16, kf, 5, layers, 12, input_kernel_size=2, seed=seed, dtype=torch.float64)
    return {k: v for k, v in sd.items() if torch.is_tensor(v)}


def _grads(fn, x, sd, cot):
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x = x.clone().requires_grad_(True)
    y = fn(x, sd)
    (y * cot).sum().backward()
    g = {k: v.grad for k, v in sd.items() if v.grad is not None}
    g["dx0"] = x.grad
    g["forward"] = y.detach()
    return g


def _assert_same(a, b):
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    for k in b:
        assert O.rel_err(a[k], b[k]) < 1e-12, (k, O.rel_err(a[k], b[k]))


def test_exact_wavenet_is_the_oracle():
    sd = _state("wavenet", LAYERS)
    g = torch.Generator().manual_seed(1)
    x, cot = torch.randn(2, 8, 40, generator=g, dtype=torch.float64), torch.randn(2, 12, 40, generator=g, dtype=torch.float64)
    want = _grads(lambda x, s: O.wavenet(x, s, LAYERS, False), x, sd, cot)
    for fused in (True, False):
        _assert_same(_grads(lambda x, s: R.wavenet(x, s, LAYERS, None, fused_head=fused), x, sd, cot), want)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("kf", [1, 3])
def test_exact_rawctcnet_is_the_oracle(causal, kf):
    layers = [(16, 16, 2, 1), (16, 16, 3, 2), (16, 16, 3, 7)]
    sd = _state("rawctc", layers, kf=kf, seed=kf)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 1, 30, generator=g, dtype=torch.float64)
    cot = torch.randn(2, 5, 30 + kf - 1, generator=g, dtype=torch.float64)
    want = _grads(lambda x, s: O.raw_ctcnet(x, s, layers, kf, 1, False, False, causal), x, sd, cot)
    for fused in (True, False):
        _assert_same(_grads(lambda x, s: R.raw_ctcnet(x, s, layers, kf, None, causal=causal, fused=fused), x, sd, cot), want)


def test_exact_stack_call_is_the_oracle():
    layers = [(16, 16, 2, 1), (16, 16, 3, 4)]
    sd = _state("wavenet", layers)
    g = torch.Generator().manual_seed(3)
    x, cot = torch.randn(2, 16, 25, generator=g, dtype=torch.float64), torch.randn(2, 12, 25, generator=g, dtype=torch.float64)
    prefixes = [("convolutions.%d." % l, "bottlenecks.%d." % l) for l in range(len(layers))]
    want = _grads(lambda x, s: O.block_stack(x, torch.zeros(2, 12, 25, dtype=torch.float64), s, layers, True)[1], x, sd, cot)
    _assert_same(_grads(lambda x, s: R.stack_call(x, s, layers, True, None, prefixes), x, sd, cot), want)


def _classifier_state(in_dim, layers, out_dim, pool, input_kwidth, input_dilation, seed):
    from wavenet_speech_amd.modules.classifier import WaveNetClassifier
    torch.manual_seed(seed)
    net = WaveNetClassifier(in_dim, 5, layers, out_dim, pool_kernel_size=pool, input_kernel_size=input_kwidth,
                            input_dilation=input_dilation, softmax=False)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape))
    return {k: v.double() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("pool,L,kw,dil", [(1, 17, 2, 1), (2, 31, 3, 2), (3, 30, 2, 3), (5, 44, 2, 1), (8, 8, 3, 1)])
def test_exact_classifier_is_the_oracle(pool, L, kw, dil):
    layers = [(16, 16, 2, 1), (16, 24, 3, 2), (24, 16, 2, 5)]
    sd = _classifier_state(7, layers, 12, pool, kw, dil, seed=pool)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 7, L, generator=g, dtype=torch.float64)
    cot = torch.randn(2, 5, L // pool, generator=g, dtype=torch.float64)
    want = _grads(lambda x, s: O.wavenet_classifier(x, s, layers, pool, dil, False), x, sd, cot)
    if L % pool:
        assert bool((want["dx0"][:, :, L - L % pool:] == 0).all())          # the dropped tail gets an exact zero
    for fused in (True, False):
        _assert_same(_grads(lambda x, s: R.wavenet_classifier(x, s, layers, pool, None, input_dilation=dil, input_kwidth=kw,
                                                              fused=fused), x, sd, cot), want)


@pytest.mark.parametrize("name", ["classifier_00"])
def test_exact_classifier_reproduces_the_golden(name):
    """forward and every gradient, x included, of the reference's own classifier run, at test_oracle_golden.py's tolerances"""
    from tests import goldenio
    from tests.goldenio import ORACLE_TOL as TOL
    g = goldenio.load(name)
    m = g.meta
    assert not m["softmax"]
    sd = {k: v.double() for k, v in g.sd.items() if v.is_floating_point()}
    got = _grads(lambda x, s: R.wavenet_classifier(x, s, m["layers"], m["pool_kernel_size"], None, input_dilation=m["input_dilation"],
                                                   input_kwidth=m["input_kernel_size"]), g.inputs["x"].double(), sd,
                 g.cots[0].double())
    assert O.rel_err(got["forward"], g.outs[0].double()) < TOL
    seen = 0
    for k, ref in g.grads.items():
        if g.hasgrad[k]:
            assert O.rel_err(got[k], ref.double()) < 1e-4, k
            seen += 1
    assert seen >= 20
    assert O.rel_err(got["dx0"], g.grad_inputs["x"].double()) < 1e-4


@pytest.mark.parametrize("mutant", R.POOL_MUTANTS)
def test_pool_mutants_differ_from_the_mean(mutant):
    """each altered pooling the GPU mutant tests use is a different operation (value or gradient), not a restatement"""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 23, generator=g, dtype=torch.float64, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    y, y2 = R.avg_pool(x, 5), R.avg_pool(x2, 5, mutant)
    assert y.shape == y2.shape == (2, 3, 4)
    y.sum().backward()
    y2.sum().backward()
    assert O.rel_err(y2, y) > 1e-2 or O.rel_err(x2.grad, x.grad) > 1e-2


@pytest.mark.parametrize("fmt,bound", [("bf16", 0.1), ("f16", 0.02)])
def test_rounding_path_stays_within_its_format(fmt, bound):
    """the rounding path differs from the exact one, by the format's error (e_fmt is what the GPU bounds are multiples of)"""
    sd = _state("wavenet", LAYERS)
    g = torch.Generator().manual_seed(4)
    x, cot = torch.randn(2, 8, 40, generator=g, dtype=torch.float64), torch.randn(2, 12, 40, generator=g, dtype=torch.float64)
    slopes = R.Pattern({})
    with torch.no_grad():
        R.wavenet(x, sd, LAYERS, fmt, slopes=slopes)
    exact = _grads(lambda x, s: R.wavenet(x, s, LAYERS, None, slopes=slopes), x, sd, cot)
    rounded = _grads(lambda x, s: R.wavenet(x, s, LAYERS, fmt, slopes=slopes), x, sd, cot)
    for k in exact:
        mx, rms = R.distances(rounded[k], exact[k])
        assert 0 < rms and mx < bound, (k, mx, rms)
