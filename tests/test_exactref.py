"""CPU: the exact references of tests/exactref.py.  For the whole case table of tests/test_gpu_exact.py: the conditions under which
any summation order is exact hold (assert_exact), and every reference agrees with the project's fp64 oracle on the same inputs to
1e-12 -- true tanh and sigmoid differ from the three-valued gate by less than 1e-13 at |x| >= 89, and the LeakyReLU pattern is
replayed from the exact reference's own pre-activations (an element that is exactly 0 takes the slope, torch's rule)."""
import pytest
import torch

from oracle import wavenet_oracle as O
from tests import exactref as X

TOL = 1e-12


def _close(got, want, name):
    assert got.shape == want.shape, name
    # (1e-30: where the exact gate gives 0 the oracle's sigmoid (1 - sigmoid) leaves e^-128 times a gradient)
    err = float((got - want).abs().max())
    assert err <= TOL * float(want.abs().max()) + 1e-30, (name, err, float(want.abs().max()))


def test_generators_and_units():
    rng = X.rng_of(0)
    t = X.dyadic(rng, (50, 7), 3, -2, 0.5)
    assert float(t.abs().max()) <= 7 / 4 and X.unit(t) >= 0.25 and 0.2 < float((t != 0).double().mean()) < 0.8
    assert X.unit(torch.tensor([6.0, 0.0, -10.0])) == 2.0 and X.unit(torch.tensor([0.375])) == 0.125
    assert X.unit(torch.zeros(3)) == 1.0
    w = X.signed_sparse(rng, 9, 20, 3)
    assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and bool(((w != 0).sum(1) == 3).all())
    v = X.two_plane(rng, (100,), -6)
    hi, lo = X.split16(v, 1.0)
    assert bool((lo != 0).all()) and torch.equal(hi + lo, v)          # fp16 alone cannot hold them, the two planes can
    assert torch.equal(X.dyadic(X.rng_of(3, 4), (5,), 4), X.dyadic(X.rng_of(3, 4), (5,), 4))
    assert X.grad_scale(torch.tensor([3.0])) == 2.0 ** -4 and X.grad_scale(torch.tensor([0.25])) == 1.0
    # an inexact product is refused
    bad = X.Case()
    X._acc(bad.products, "p", [(torch.matmul, (torch.full((1, 3), 2.0 ** 23 + 1), torch.ones(3, 1)))])
    with pytest.raises(AssertionError):
        X.assert_exact(bad)
    bad = X.Case()
    X._acc(bad.products, "p", [(torch.matmul, (torch.ones(1, 1), torch.ones(1, 1)))])
    bad.gates.append(("g", torch.tensor([64.0]), torch.tensor([0.0])))
    with pytest.raises(AssertionError):
        X.assert_exact(bad)


def test_gate3_is_the_limit_of_the_true_gate():
    a = torch.tensor([-256.0, -128.0, 0.0, 128.0, 384.0], dtype=X.DT)
    ta, sg = X.gate3(a, a)
    assert float((ta - torch.tanh(a)).abs().max()) < 1e-13 and float((sg - torch.sigmoid(a)).abs().max()) < 1e-13


@pytest.mark.parametrize("case", X.CONV_CASES + [None])
def test_conv_reference(case):
    c = X.conv_case(X.CONV_NO_BIAS, False) if case is None else X.conv_case(case)
    X.assert_exact(c)
    x, w = c.x.clone().requires_grad_(True), c.w.clone().requires_grad_(True)
    b = None if c.b is None else c.b.clone().requires_grad_(True)
    y = O.dilated_conv(x, w, b, c.d, c.causal)
    (y * c.dy).sum().backward()
    _close(c.ref["y"], y.detach(), "y")
    _close(c.ref["dx"], x.grad, "dx")
    _close(c.ref["dw"], w.grad, "dw")
    if b is not None:
        _close(c.ref["db"], b.grad, "db")
    _close(c.ref["y"], O.dilated_conv(c.x, c.w, c.b, c.d, c.causal, impl="aten"), "aten")
    if case == (2, 33, 40, 2, 200, True, 128):
        assert float(c.ref["dw"][:, :, 0].abs().max()) == 0.0 and float(c.ref["dw"][:, :, 1].abs().max()) > 0.0


@pytest.mark.parametrize("cls", X.HALF_CLASSES)
@pytest.mark.parametrize("case", X.HALF_CONV_CASES)
def test_f16x3_conv_split_is_exact(case, cls):
    """nothing leaves fp16's range, the emulated three-product result equals the integer result, the fp32 accumulation bound
    holds; and the operand the class names does need its low plane"""
    c = X.half_conv_case(case, cls)
    X.assert_exact(c)
    assert c.products.hscale and len(c.products.half) >= 12 * c.w.shape[2] + 1
    needs = {"x": (c.x, X.RS), "w": (c.w, X.WS / X.RS), "dy": (c.dy, c.dyn)}
    for name, (t, s) in needs.items():
        lo = X.split16(t, s)[1]
        assert bool((lo != 0).any()) == (name == cls), (name, cls)
    if cls == "w":
        assert bool((X.split16(c.w, X.WS)[1] != 0).any())        # the backward-data packing of the weights too
    y = O.dilated_conv(c.x, c.w, c.b, c.d, c.causal)
    _close(c.ref["y"], y, "y")


@pytest.mark.parametrize("mode", X.GATE_MODES)
@pytest.mark.parametrize("case", X.BLOCK_CASES)
def test_block_reference(case, mode):
    c = X.block_case(case, mode)
    X.assert_exact(c)
    if mode == "mixed":
        assert len(c.pairs) >= c.want_pairs and c.want_pairs >= 8, sorted(c.pairs)
        assert float(c.ref["da"].abs().max()) > 0 and (c.want_pairs < 9 or float(c.ref["dg"].abs().max()) > 0)
    else:
        assert c.pairs <= {(t, s) for t in (-1.0, 1.0) for s in (0.0, 1.0)}
        assert float(c.ref["da"].abs().max()) == 0 and float(c.ref["dg"].abs().max()) == 0
    x = c.x.clone().requires_grad_(True)
    p = {k: v.clone().requires_grad_(True) for k, v in c.p.items()}
    r, s, (ta, sg, z) = O.residual_block(x, p, c.d, c.causal, return_saved=True)
    (r * c.dr).sum().backward(retain_graph=True)
    (s * c.ds).sum().backward()
    for name, t in (("r", r), ("s", s), ("sg", sg), ("z", z)):
        _close(c.ref[name], t.detach(), name)
    _close(c.ref["dx"], x.grad, "dx")
    for k in O.BLOCK_KEYS:
        _close(c.ref[k], p[k].grad, k)
    dx, grads = O.residual_block_backward(c.x, c.p, c.d, c.causal, c.dr, c.ds)      # the hand-derived rule as well
    _close(c.ref["dx"], dx, "dx (hand-derived)")
    for k in O.BLOCK_KEYS:
        _close(c.ref[k], grads[k], k)


def _oracle_grads(c, y, sd, x):
    (y * c.cot).sum().backward()
    got = {"forward": y.detach(), "dx0": x.grad}
    got.update({k: v.grad for k, v in sd.items() if v.grad is not None})
    return got


@pytest.mark.parametrize("L", X.LENGTHS)
@pytest.mark.parametrize("stack", sorted(X.STACKS))
def test_stack_reference(stack, L):
    c = X.stack_case(stack, L)
    X.assert_exact(c)
    assert len(c.pairs) == 9, sorted(c.pairs)
    sd = {k: v.clone().requires_grad_(True) for k, v in c.sd.items()}
    x = c.x.clone().requires_grad_(True)
    _, y = O.block_stack(x, torch.zeros(X.B, X.MS, L, dtype=X.DT), sd, c.layers, True)
    got = _oracle_grads(c, y, sd, x)
    want = {k: v for k, v in c.ref.items() if k in got}
    assert set(want) == set(got), sorted(set(want) ^ set(got))
    for k in got:
        _close(want[k], got[k], k)
    n = len(c.layers)
    assert "convolutions.%d.residual_proj.weight" % (n - 1) not in got            # the last residual output is unused
    assert float(c.ref["dx0"].abs().max()) > 0
    for l in range(n):
        top = l >= n - 2                          # the blocks whose gates are not saturated
        assert (float(c.ref["convolutions.%d.conv_tanh.conv1d.weight" % l].abs().max()) > 0) == top
        assert float(c.ref["convolutions.%d.conv1x1_skip.weight" % l].abs().max()) > 0
        if not top:
            assert float(c.ref["convolutions.%d.residual_proj.weight" % l].abs().max()) > 0


def test_f16x3_stack_grid_is_exact():
    """an f16x3 stack whose every product is exact: the residual stream on the grid 128 (the packed gate weights must stay below
    16, so the multiples of Q come from the inputs, the biases and the residual weights), every stored tensor held by its two
    fp16 planes at the scale the half path stores it with, one operand of every product with an empty low plane"""
    c = X.stack_case("three_k2", 130, False, True)
    X.assert_exact(c)
    assert len(c.pairs) == 9 and c.products.hscale and c.dyn == X.grad_scale(c.cot)
    assert len(c.products.half) > 200 and all(ok for _n, ok, _w in c.products.half)
    for k, v in c.sd.items():
        if "conv_tanh" in k or "conv_sigmoid" in k or "residual_proj.weight" in k:
            assert float(v.abs().max()) * X.WS / X.RS <= 65504.0 or k.endswith("bias"), k
    sd = {k: v.clone().requires_grad_(True) for k, v in c.sd.items()}
    x = c.x.clone().requires_grad_(True)
    _, y = O.block_stack(x, torch.zeros(X.B, X.MS, 130, dtype=X.DT), sd, c.layers, True)
    got = _oracle_grads(c, y, sd, x)
    for k in got:
        _close(c.ref[k], got[k], k)
    assert float(c.ref["convolutions.2.conv_tanh.conv1d.weight"].abs().max()) > 0 and float(c.ref["dx0"].abs().max()) > 0


@pytest.mark.parametrize("stack,L", X.NET_CASES)
def test_net_reference(stack, L):
    c = X.stack_case(stack, L, net=True)
    X.assert_exact(c)
    assert len(c.pairs) == 9, sorted(c.pairs)
    assert c.zero_row_is_zero
    assert bool((c.slopes["output_stack.0"] == X.SLOPES[0]).any()) and bool((c.slopes["output_stack.0"] == 1).any())
    sd = {k: v.clone().requires_grad_(True) for k, v in c.sd.items()}
    x = c.x.clone().requires_grad_(True)
    y = O.wavenet(x, sd, c.layers, False, slopes=c.slopes)
    got = _oracle_grads(c, y, sd, x)
    want = {k: v for k, v in c.ref.items() if k in got}
    assert set(want) == set(got), sorted(set(want) ^ set(got))
    for k in got:
        _close(want[k], got[k], k)
    # the zero row of skips_sum passes slope * gradient: its bottleneck bias gradients are non-zero
    assert float(c.ref["bottlenecks.0.bias"][X.ZERO_ROW].abs()) > 0
    assert float(c.ref["entry_conv1d.conv1d.weight"].abs().max()) > 0 and float(c.ref["dx0"].abs().max()) > 0


def test_first_difference():
    a = torch.zeros(2, 3)
    b = a.clone()
    assert X.first_difference(a, b) is None
    b[1, 2] = 1e-30
    assert X.first_difference(a, b)[0] == (1, 2)
