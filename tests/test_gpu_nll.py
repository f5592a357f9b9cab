"""GPU: the fused NLL head (csrc/wn_nll.hip through functional.sequence_nll) against fp64, at its edges.

Reference: fp64 logsumexp minus the gathered logit, summed over time and batch and divided by B; gradient (softmax - onehot) g / B.
Bars (the project's own, from test_fused_nll_head_matches_the_reference_loop, now against fp64 instead of torch's fp32):
loss 1e-5 max(1, |loss|), gradient 1e-6 max(1, max|grad|) + 1e-7.  The measured distances are printed."""
import math

import pytest
import torch

from wavenet_speech_amd import functional as HF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def reference(logits, target, g, got_grad=None):
    """(loss, max|grad|, max|got_grad - grad|) in fp64, one utterance at a time (the largest case holds 65 M logits)"""
    B, C, L = logits.shape
    loss, gmax, err = 0.0, 0.0, 0.0
    for b in range(B):
        x = logits[b].double()
        lse = torch.logsumexp(x, dim=0)
        loss += float((lse - x.gather(0, target[b].unsqueeze(0))[0]).sum())
        p = torch.exp(x - lse)
        p.scatter_add_(0, target[b].unsqueeze(0), -torch.ones(1, L, dtype=torch.float64))
        p *= g / B
        gmax = max(gmax, float(p.abs().max()))
        if got_grad is not None:
            err = max(err, float((got_grad[b].double() - p).abs().max()))
    return loss / B, gmax, err


def hip(logits, target, g):
    x = logits.to(DEV).requires_grad_(True)
    loss = HF.sequence_nll(x, target.to(DEV))
    (loss * g).backward()
    return loss.detach(), x.grad.cpu()


def check(label, logits, target, g=1.0):
    loss, grad = hip(logits, target, g)
    want, gmax, err = reference(logits, target, g, grad)
    assert math.isfinite(want), (label, want)
    dl = abs(float(loss) - want)
    print("nll %-40s B %2d C %3d L %5d g %.4g: loss %.9g (fp64 %.9g) rel %.2e; grad err %.2e of max %.2e"
          % (label, logits.shape[0], logits.shape[1], logits.shape[2], g, float(loss), want, dl / max(1.0, abs(want)), err, gmax))
    assert bool(torch.isfinite(grad).all()), label
    assert dl < 1e-5 * max(1.0, abs(want)), (label, float(loss), want)
    assert err < 1e-6 * max(1.0, gmax) + 1e-7, (label, err, gmax)
    return loss, grad


def _randn(B, C, L, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, L, generator=g) * scale, torch.randint(0, C, (B, L), generator=g)


@pytest.mark.parametrize("L", [1, 3, 4, 5, 1023, 1024, 1025])
@pytest.mark.parametrize("C", [1, 2, 5, 256, 257])
def test_shapes_vs_fp64(C, L):
    """L % 4 == 0 takes the 16-byte loads, every other L the scalar path; L = 1024, 1025 cross a 256-thread workgroup at B = 1;
    B ceil(L / 4) < 64 for L <= 5 leaves idle lanes in the wave and workgroup folds"""
    for B in (1, 3):
        x, t = _randn(B, C, L, seed=1000 * C + L + B)
        check("shape", x, t, g=1.7)


def test_full_size_head_vs_fp64():
    """configs[2]'s head: 16 x 256 x 16000, forward and backward"""
    x, t = _randn(16, 256, 16000, seed=7)
    check("full size", x, t, g=1.0 / 16000)


def _wide(B, C, L, seed):
    """logits over +-80, the largest of each frame (80) in the first, a middle or the last class by turns: the running maximum is
    replaced late (the online rescale branch), early, or in between"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, C, L, generator=g) * 2 - 1) * 79.0
    where = torch.tensor([0, C // 2, C - 1])[torch.arange(L) % 3]
    x.scatter_(1, where.view(1, 1, L).expand(B, 1, L), 80.0)
    return x, torch.randint(0, C, (B, L), generator=g)


@pytest.mark.parametrize("B,C,L", [(1, 5, 7), (3, 256, 300), (1, 257, 1025), (3, 2, 64)])
@pytest.mark.parametrize("g", [1.0, 1.7, None])
def test_wide_logits_and_upstream_factor(B, C, L, g):
    x, t = _wide(B, C, L, seed=B + C + L)
    check("+-80", x, t, g=1.0 / L if g is None else g)
    x2, t2 = _randn(B, C, L, seed=L)
    check("randn x 3", x2, t2, g=1.0 / L if g is None else g)


@pytest.mark.parametrize("B,C,L", [(1, 5, 4), (3, 256, 9), (1, 1, 3)])
def test_equal_logits(B, C, L):
    x, t = _randn(B, C, L, seed=3)
    x[:, :, 0] = 2.5
    x[:, :, L - 1] = -80.0
    loss, grad = check("equal", x, t)
    assert float((grad[:, :, 0] * B + torch.nn.functional.one_hot(t[:, 0], C) - 1.0 / C).abs().max()) < 1e-6


@pytest.mark.parametrize("B,C,L", [(1, 5, 4), (3, 256, 9), (2, 33, 1025)])
def test_one_huge_logit(B, C, L):
    """one class at 1e30, the others of order 1: target on the huge class in one frame (loss 0 there), on a small class in another
    (loss 1e30: representable, as is the gradient +-1 / B)"""
    x, t = _randn(B, C, L, seed=4, scale=1.0)
    x[:, 1, 0] = 1e30
    t[:, 0] = 1
    check("1e30, target on it", x, t)
    x[:, C - 1, L - 1] = 1e30
    t[:, L - 1] = 0
    loss, grad = check("1e30, target beside it", x, t)
    assert float(grad[0, C - 1, L - 1]) == pytest.approx(1.0 / B, rel=1e-6) and float(grad[0, 0, L - 1]) == pytest.approx(-1.0 / B, rel=1e-6)


@pytest.mark.parametrize("where", ["first", "middle", "last", "first two", "all but the last"])
@pytest.mark.parametrize("B,C,L", [(1, 5, 4), (3, 256, 9), (2, 33, 1025)])
def test_masked_classes(B, C, L, where):
    """classes at -inf with the target on a finite class: a finite loss and an exact zero gradient on the masked classes, as
    torch.nn.functional.cross_entropy gives -- whatever the position (class 0 is where the online maximum is still -inf)"""
    idx = {"first": [0], "middle": [C // 2], "last": [C - 1], "first two": [0, 1], "all but the last": list(range(C - 1))}[where]
    x, t = _randn(B, C, L, seed=5)
    frames = torch.arange(L) % 2 == 0                     # every other frame is masked, the rest are ordinary
    free = [c for c in range(C) if c not in idx]
    for c in idx:
        x[:, c, frames] = -math.inf
    t[:, frames] = torch.tensor(free)[torch.randint(0, len(free), (B, int(frames.sum())), generator=torch.Generator().manual_seed(6))]
    loss, grad = check("-inf " + where, x, t, g=1.7)
    for c in idx:
        assert bool((grad[:, c, frames] == 0).all())
    xc = x.clone().requires_grad_(True)
    (torch.nn.functional.cross_entropy(xc, t, reduction="sum") / B * 1.7).backward()
    assert bool(torch.isfinite(xc.grad).all()) and all(bool((xc.grad[:, c, frames] == 0).all()) for c in idx)   # (torch's own)


def test_masked_target_gives_an_infinite_loss():
    """a target that is itself masked: +inf, as torch.nn.functional.cross_entropy gives"""
    x, t = _randn(2, 7, 10, seed=8)
    x[1, 3, 4] = -math.inf
    t[1, 4] = 3
    want = torch.nn.functional.cross_entropy(x, t, reduction="sum") / 2
    got = HF.sequence_nll(x.to(DEV), t.to(DEV))
    assert float(want) == math.inf and float(got) == math.inf


@pytest.mark.parametrize("B,C,L", [(3, 256, 1025), (1, 5, 3), (16, 64, 4096)])
def test_two_calls_give_equal_bits(B, C, L):
    x, t = _wide(B, C, L, seed=9)
    a, ga = hip(x, t, 1.7)
    b, gb = hip(x, t, 1.7)
    assert torch.equal(a, b) and torch.equal(ga, gb)
