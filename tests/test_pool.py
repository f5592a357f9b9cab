"""The AvgPool1d kernels of csrc/wn_front.hip on their own -- pool_load_kernel (wn_series_load_pooled), hpool_load_kernel<P,BF>
(wn_hseries_load_pooled) and pool_unload_kernel (wn_pool_backward) -- through the C ABI, with series buffers leased the way the
stack leases them (series.Lease, functional_half._hlease).  No stack is involved.

What the layouts promise (series.py lines 2-4), and what is therefore asserted of a load of Lp = L // pool
pooled steps into a buffer pre-filled with a sentinel:
  * fp32 series [B][Cp][ld]: everything outside the valid window -- rows c >= C, columns < halo and columns >= halo + Lp -- is zero
    and STAYS as it was: a kernel writes the valid window [C][halo, halo + Lp) only.  Here: the sentinel is unchanged there.
  * half series [B][P][G][ld][8]: the same for the columns; inside the window a 16-byte unit holds 8 channels and is written whole,
    so the pad channels c >= C (the rest of a partly filled group of 8, and the groups that pad C to a multiple of 32) are written,
    and must be exactly +0 -- they are K rows of every GEMM that reads the series.

The CPU test checks, for the inputs the GPU test uses, that fp32 arithmetic as the kernel does it (sum in order, one multiply by
fp32(1 / (16 pool)), one rounding) differs from the fp64 mean rounded once in well under the 1 % of elements the GPU test allows."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import halfref as R

DEV = "cuda:0"
POOLS = (1, 2, 3, 5, 8)
SENTINEL = -768.0        # exact in fp32, fp16 and bf16


def lengths(pool):
    """(L // pool, L % pool): one pooled step; 257 = one past a 256-column tile of the half layout; 129 = one past a 128-column
    tile of the fp32 layout; tails of 0, 1 and pool - 1"""
    rems = sorted({0, min(1, pool - 1), pool - 1})
    out = [(1, rems[-1]), (1, 0), (257, rems[len(rems) // 2]), (129, rems[-1]), (257, 0), (40, rems[0])]
    return [(lp, r, lp * pool + r) for lp, r in out]


def half_inputs(B, C, L, seed):
    return torch.randn(B, C, L, generator=torch.Generator().manual_seed(seed))


HALF_SHAPES = [(3, 33, 257), (1, 5, 1), (2, 12, 129), (1, 64, 40), (1, 256, 129)]       # B, C, L // pool


def emulate_half_load(x, pool, fmt):
    """the kernel's arithmetic in fp32: sum the window in order, multiply once by fp32(scale / pool), round once: (the fp32 value as
    stored, mean / 16; its rounding to the format)"""
    B, C, L = x.shape
    Lp = L // pool
    w = x[:, :, :Lp * pool].reshape(B, C, Lp, pool)
    acc = torch.zeros(B, C, Lp)
    for q in range(pool):
        acc = acc + w[:, :, :, q]
    s = torch.tensor(R.RS, dtype=torch.float32) / torch.tensor(float(pool), dtype=torch.float32)
    v = acc * s
    return v, v.to(torch.bfloat16 if fmt == "bf16" else torch.float16)


def reference_half_load(x, pool, fmt):
    """the fp64 mean stored once at RS, in the format (the stored halves)"""
    avg = F.avg_pool1d(x.double(), pool)
    return (avg * R.RS).to(torch.bfloat16 if fmt == "bf16" else torch.float16)


def ulp_distance(a, b):
    """distance in units of the last place between two half tensors of the same format (sign-magnitude keys: -0 and +0 coincide)"""
    def key(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        mag = bits & 0x7FFF
        return torch.where(bits >= 0x8000, -mag, mag)
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_fp32_arithmetic_stays_under_the_one_percent_cap(fmt):
    worst = 0.0
    for pool in POOLS:
        for B, C, Lp in HALF_SHAPES:
            if B * C * Lp < 1000:
                continue                     # (a handful of elements: one boundary case would be percents; they are held to 1 ulp only)
            x = half_inputs(B, C, Lp * pool + pool - 1, seed=pool * 1000 + C)
            d = ulp_distance(emulate_half_load(x, pool, fmt)[1], reference_half_load(x, pool, fmt))
            assert int(d.max()) <= 1
            worst = max(worst, float((d != 0).float().mean()))
    print("fp32 emulation of the %s pooled load differs from the fp64 reference in at most %.4f %% of the elements" % (fmt, 100 * worst))
    assert worst < 0.002                     # a fifth of the cap; a truncating or twice-rounding kernel differs in tens of percent


def _lib_and_helpers():
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd.functional import _p, _stream
    return _lib.load(), _lib, _p, _stream


@pytest.mark.gpu
@pytest.mark.parametrize("pool", POOLS)
def test_pool_backward_is_one_division_and_writes_every_element(pool):
    lib, _lib, _p, _stream = _lib_and_helpers()
    shapes = [(1, 1), (3, 7), (1, 64), (3, 64), (1, 7), (3, 1)]
    for i, (Lp, rem, L) in enumerate(lengths(pool)):
        B, C = shapes[i % len(shapes)]
        g = torch.Generator().manual_seed(L + C)
        dp = torch.randn(B, C, Lp, generator=g).to(DEV)
        dx = torch.full((B, C, L), float("nan"), device=DEV)
        _lib.check(lib.wn_pool_backward(_p(dp), _p(dx), B, C, L, pool, _stream()), "wn_pool_backward")
        torch.cuda.synchronize()
        # one IEEE fp32 division per element: formed on the CPU with a tensor divisor (torch divides a device tensor by a SCALAR as a
        # multiplication by its reciprocal, which is not the correctly rounded quotient for pool = 3, 5)
        rep = dp.cpu().repeat_interleave(pool, dim=2)
        want = rep / torch.full_like(rep, float(pool))
        assert torch.equal(dx[:, :, :Lp * pool].cpu(), want), (pool, B, C, L)
        tail = dx[:, :, Lp * pool:]
        assert tail.shape[2] == rem and bool((tail == 0).all()) and not bool(torch.signbit(tail).any()), (pool, B, C, L)


@pytest.mark.gpu
@pytest.mark.parametrize("pool", POOLS)
def test_fp32_pooled_load_vs_fp64_and_writes_the_valid_window_only(pool):
    from wavenet_speech_amd.series import Lease, SeriesLayout
    lib, _lib, _p, _stream = _lib_and_helpers()
    shapes = [(1, 1), (3, 7), (1, 64), (3, 33), (1, 12), (3, 5)]
    for i, (Lp, rem, L) in enumerate(lengths(pool)):
        B, C = shapes[i % len(shapes)]
        x = torch.randn(B, C, L, generator=torch.Generator().manual_seed(L * 7 + C)) * 3
        layout = SeriesLayout(Lp, 4)
        lease = Lease(B, C, layout, DEV)
        try:
            lease.t.fill_(SENTINEL)
            _lib.check(lib.wn_series_load_pooled(_p(x.to(DEV)), _p(lease), B, C, L, pool, layout.ld, layout.halo, _stream()),
                       "wn_series_load_pooled")
            torch.cuda.synchronize()
            buf = lease.t.cpu()
        finally:
            lease.t.zero_()                  # the pool's invariant: a buffer goes back zero outside its window (and here inside too)
        h = layout.halo
        assert buf.shape == (B, (C + 7) // 8 * 8, layout.ld) and h >= 4
        got = buf[:, :C, h:h + Lp]
        # error of one element: pool - 1 additions and one division in fp32, first order: pool 2^-24 mean|x| over its window
        bound = pool * 2.0 ** -24 * F.avg_pool1d(x.double().abs(), pool)
        err = (got.double() - F.avg_pool1d(x.double(), pool)).abs()
        assert bool((err <= bound).all()), (pool, B, C, L, float((err / bound).max()))
        outside = buf.clone()
        outside[:, :C, h:h + Lp] = SENTINEL
        assert bool((outside == SENTINEL).all()), (pool, B, C, L)


def _half_load(precision, x, pool, flag=None):
    """(planes [B][P][G][ld][8] on the CPU, layout) of wn_hseries_load_pooled into a sentinel-filled leased buffer"""
    from wavenet_speech_amd import functional_half as FH
    lib, _lib, _p, _stream = _lib_and_helpers()
    B, C, L = x.shape
    mode = FH._Mode(precision)
    layout = FH.HalfLayout(L // pool, 4)
    lease = FH._hlease(mode, B, C, layout, DEV)
    try:
        lease.t.fill_(SENTINEL)
        _lib.check(lib.wn_hseries_load_pooled(mode.code, _p(x.to(DEV)), _p(lease), B, C, L, pool, layout.ld, layout.halo,
                                              ctypes.c_float(float(lib.wn_hseries_residual_scale())), None, _p(flag), _stream()),
                   "wn_hseries_load_pooled")
        torch.cuda.synchronize()
        buf = lease.t.cpu()
    finally:
        lease.t.zero_()
    G = (C + 31) // 32 * 4
    return buf.view(B, mode.planes, G, layout.ld, 8), layout


def _window(planes, layout, Lp, C):
    """[B][P][C'][Lp] from the unit layout, C' = 8 G channels (pads included)"""
    B, P, G, ld, _ = planes.shape
    return planes[:, :, :, layout.halo:layout.halo + Lp, :].permute(0, 1, 2, 4, 3).reshape(B, P, G * 8, Lp)


@pytest.mark.gpu
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_half_pooled_load_vs_fp64_rounded_once(precision, pool):
    for B, C, Lp in HALF_SHAPES:
        for rem in sorted({0, pool - 1}):
            L = Lp * pool + rem
            x = half_inputs(B, C, L, seed=pool * 1000 + C)
            planes, layout = _half_load(precision, x, pool)
            assert float(lib_rs()) == R.RS and layout.halo >= 8
            w = _window(planes, layout, Lp, C)
            got = w[:, 0, :C]
            d = ulp_distance(got, reference_half_load(x, pool, precision))
            frac = float((d != 0).float().mean())
            print("%s pooled load pool %d B %d C %3d L %4d: %.4f %% of the elements 1 ulp from the fp64 reference" % (precision, pool, B, C, L, 100 * frac))
            assert int(d.max()) <= 1, (precision, pool, B, C, L)
            if got.numel() >= 1000:
                assert frac <= 0.01, (precision, pool, B, C, L, frac)
            pads = w[:, 0, C:]
            assert bool((pads.contiguous().view(torch.int16) == 0).all()), "pad channels must be +0"
            outside = planes.clone()
            outside[:, :, :, layout.halo:layout.halo + Lp, :] = SENTINEL
            assert bool((outside == SENTINEL).all()), (precision, pool, B, C, L)


def lib_rs():
    return _lib_and_helpers()[0].wn_hseries_residual_scale()


@pytest.mark.gpu
@pytest.mark.parametrize("pool", POOLS)
def test_f16x3_pooled_load_carries_22_bits(pool):
    """inputs of order 1 (2 <= |x| < 8, one sign per row, so that the means are too): both planes then lie in fp16's normal range or
    at its edge, and hi + lo reproduces the fp32 value to 2^-21 relative (two 11-bit planes carry 22 bits, one bit of margin)"""
    for B, C, Lp in HALF_SHAPES:
        L = Lp * pool + pool - 1
        g = torch.Generator().manual_seed(pool + C)
        x = (2 + 6 * torch.rand(B, C, L, generator=g)) * (torch.randint(0, 2, (B, C, 1), generator=g) * 2 - 1)
        planes, layout = _half_load("f16x3", x, pool)
        w = _window(planes, layout, Lp, C)
        v32 = emulate_half_load(x, pool, "f16")[0].double()
        got = w[:, 0, :C].double() + w[:, 1, :C].double()
        rel = float(((got - v32).abs() / v32.abs()).max())
        print("f16x3 pooled load pool %d B %d C %3d L %4d: hi + lo within %.2e of the fp32 value" % (pool, B, C, L, rel))
        assert rel <= 2.0 ** -21, (pool, B, C, L, rel)
        assert bool((w[:, :, C:].contiguous().view(torch.int16) == 0).all()), "pad channels must be +0 in both planes"
        outside = planes.clone()
        outside[:, :, :, layout.halo:layout.halo + Lp, :] = SENTINEL
        assert bool((outside == SENTINEL).all())


@pytest.mark.gpu
def test_pooled_load_beyond_fp16_raises_the_overflow_flag():
    """|mean| / 16 > 65504 is out of fp16's range: the store-side check sets the flag in the fp16 modes; bf16 has fp32's range"""
    x = torch.randn(2, 12, 90, generator=torch.Generator().manual_seed(1))
    x[1, 3, 30:33] = 2.0e6
    for precision, want in (("f16", 1), ("f16x3", 1), ("bf16", 0)):
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        planes, layout = _half_load(precision, x, 3, flag)
        assert int(flag.item()) == want, precision
        if precision == "bf16":
            assert float(_window(planes, layout, 30, 12)[1, 0, 3, 10]) * 16 == pytest.approx(2.0e6, rel=2.0 ** -8)
