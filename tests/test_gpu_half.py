"""GPU parity of the half-precision-MFMA modes of the residual stack (wavenet_speech_amd.set_precision).

f16x3 (three-product fp16 split, fp32 accumulate) is held to the SAME 1e-4 bar as the exact-fp32 path, forward and every
gradient, on the golden fixtures and against the oracle.  Plain f16 / bf16 (BASELINE configs[4] / configs[1]) are held to the
error their storage format implies: tests/halfref.py evaluates the model in fp64, rounding every tensor the half path stores, and
every compared tensor must satisfy e_hip <= KAPPA e_fmt + FLOOR in max-norm and RMS (e_hip: the HIP result's distance from exact
fp64, e_fmt: the rounding reference's).  The measured distances are printed."""
import pytest
import torch

import wavenet_speech_amd as W
from oracle import wavenet_oracle as O
from tests import goldenio
from tests import halfref as R
from tests.gpu_stack import PLAIN, TOL, condition as _condition, cycles_of as _layers, launched as _launched, onehot as _onehot
from tests.gpu_stack import properties as _properties, run_golden as _run_golden, wavenet as _wavenet
from tests.gpu_util import DEV
from wavenet_speech_amd import functional as HF

pytestmark = pytest.mark.gpu


def _cond_wavenet(c, layers, in_dim=None, seed=0, out_dim=None):
    from wavenet_speech_amd.modules.wavenet import WaveNet
    torch.manual_seed(seed)
    net = WaveNet(in_dim or c, 2, layers, out_dim or c, softmax=False)
    _condition(net)
    return net


def _cond_rawctc(c, layers, causal, seed, feature_kwidth=3, out_dim=None, input_kwidth=2, slope=0.01):
    from wavenet_speech_amd.modules.raw_ctcnet import RawCTCNet
    torch.manual_seed(seed)
    net = RawCTCNet(c, feature_kwidth, 5, layers, out_dim or c, input_kernel_size=input_kwidth, softmax=False, causal=causal)
    if slope != 0.01:
        for m in net.modules():
            if isinstance(m, torch.nn.LeakyReLU):
                m.negative_slope = slope
    return _condition(net)


def _half_ref(net, precision, slopes, layers_override=None):
    """fn(x, sd, fmt) of tests/halfref.py for `net` as the half path runs it (layers_override: other (ci, co, k, d) per block)"""
    from wavenet_speech_amd.modules.block import fusable_head
    from wavenet_speech_amd.modules.raw_ctcnet import RawCTCNet
    if isinstance(net, RawCTCNet):
        fused = fusable_head(net.output_block, precision) is not None
        layers = layers_override or [(b.in_channels, b.out_channels, b.kernel_width, b.dilation) for b in net.convolutions]
        ib = net.input_block
        return lambda x, sd, fmt: R.raw_ctcnet(x, sd, layers, net.feature_layer[0].kernel_size[0], fmt, causal=net.causal,
                                               input_dilation=ib.dilation, input_kwidth=ib.kernel_width, slopes=slopes,
                                               fused=fused)
    fused = fusable_head(net.output_stack, precision) is not None
    layers = layers_override or [(b.in_channels, b.out_channels, b.kernel_width, b.dilation) for b in net.convolutions]
    return lambda x, sd, fmt: R.wavenet(x, sd, layers, fmt, slopes=slopes, fused_head=fused)


def _run(net, x, cot, layers, precision, tol=None, replay_slopes=True, input_grad=True, kernels=None, label="", mutants=None):
    """forward and backward of `net` on the GPU in `precision` against the oracle: f16x3 at `tol` (fp32 oracle), the plain modes
    against tests/halfref.py (predicate e_hip <= KAPPA e_fmt + FLOOR).  kernels(launched) asserts the kernels the case exists to
    exercise (HF.profile_read() of the GPU forward and backward).  mutants: {name: (state dict, layers or None)} -- references
    built from altered parameters, each of which the predicate must REJECT for the unaltered GPU result.
    The LeakyReLU pattern replayed by the references is the GPU's.  f16x3: O.capture_leaky_slopes.  Plain modes: one extra forward
    on the training path (the one the measured forward takes) with the output block outside the stack function (WN_SERIES_HEAD=0:
    its convs store the same pre-activations, its LeakyReLUs become modules whose inputs a hook reads); a fused feature layer stays
    fused there -- run outside, it would round the signal and its weights where the fused layer does not -- and its own masks are
    recorded by the rounding reference (halfref.Pattern), whose rounding is the GPU's."""
    sd = {k: v.clone().requires_grad_(True) for k, v in net.state_dict().items()}
    frozen = {k for k, p in net.named_parameters() if not p.requires_grad}
    net = net.to(DEV)
    W.set_precision(net, precision)
    xg = x.to(DEV).requires_grad_(input_grad)
    front = None
    if precision in PLAIN and hasattr(net, "feature_layer"):
        from wavenet_speech_amd.modules.block import fusable_front
        front = fusable_front(net.feature_layer, precision, xg)
    if precision not in PLAIN:
        slopes, remove = O.capture_leaky_slopes(net)
    else:
        import os
        slopes, handles = {}, []
        for name, mod in net.named_modules():
            if isinstance(mod, torch.nn.LeakyReLU):
                def hook(_m, inp, name=name, ns=mod.negative_slope):
                    xin = inp[0].detach()
                    slopes[name] = torch.where(xin > 0, torch.ones_like(xin), torch.full_like(xin, ns)).cpu()
                handles.append(mod.register_forward_pre_hook(hook))
        old = os.environ.get("WN_SERIES_HEAD")
        os.environ["WN_SERIES_HEAD"] = "0"
        try:
            net(xg.detach().requires_grad_(input_grad))
        finally:
            if old is None:
                del os.environ["WN_SERIES_HEAD"]
            else:
                os.environ["WN_SERIES_HEAD"] = old
            for h in handles:
                h.remove()
        remove = lambda: None
    HF.profile_reset()
    HF.profile_enable(True)
    try:
        y1 = net(xg)
        remove()
        (y1 * cot.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        HF.profile_enable(False)
    launched = _launched()
    if kernels is not None:
        assert kernels(launched), launched
    if precision in PLAIN:
        hip = {"forward": y1.detach().cpu()}
        if input_grad:
            hip["dx0"] = xg.grad.cpu()
        for k, p in net.named_parameters():
            if k in frozen or p.grad is None:     # (the last block's residual path does not reach the output)
                continue
            hip[k] = p.grad.cpu()
        xr = x.clone().requires_grad_(input_grad)
        if front is not None:
            head = dict(slopes)
            slopes = R.Pattern({n: m.negative_slope for n, m in net.named_modules() if isinstance(m, torch.nn.LeakyReLU)})
            slopes.update(head)
            with torch.no_grad():
                _half_ref(net, precision, slopes)(xr.detach().double(), {k: v.detach().double() for k, v in sd.items()}, precision)

        def refs(base, lay):
            fn = _half_ref(net, precision, slopes if replay_slopes else None, lay)
            res = {}
            for fmt in (None, precision):
                y, g = R.run(fn, [xr], base, cot, fmt)
                assert set(g) - set(frozen) == set(hip) - {"forward"}, sorted(set(g) ^ set(hip))   # the same tensors get gradients
                g["forward"] = y
                res[fmt] = {k: g[k] for k in hip}
            return res
        res = refs(sd, None)
        out = R.check("%s%s" % (precision, label), hip, res[precision], res[None])
        for name, (sd2, lay2) in (mutants or {}).items():
            r2 = refs(sd2, lay2)
            got = R.compare("%s%s mutant %s" % (precision, label, name), hip, r2[precision], r2[None], quiet=True)
            bad = sorted(k for k, v in got.items() if not v[2])
            print("%s%s mutant %s: rejected by %d of %d tensors, e.g. %s" % (precision, label, name, len(bad), len(got), bad[:3]))
            assert bad, "mutant %s passes the predicate" % name
        return out
    xr = x.clone().requires_grad_(True)
    y0 = O.wavenet(xr, sd, layers, False, slopes=slopes if replay_slopes else None)
    (y0 * cot).sum().backward()
    errs = {"forward": O.rel_err(y1.detach().cpu(), y0), "dx": O.rel_err(xg.grad.cpu(), xr.grad)}
    for k, p in net.named_parameters():
        if sd[k].grad is None:
            assert p.grad is None, k
            continue
        errs[k] = O.rel_err(p.grad.cpu(), sd[k].grad)
    worst = max(errs, key=errs.get)
    print("%s: forward %.2e, dx %.2e, worst gradient %s %.2e" % (precision, errs["forward"], errs["dx"], worst, errs[worst]))
    assert errs[worst] < tol, (worst, errs[worst])
    return errs


@pytest.mark.parametrize("shape", [(32, 4, 300, 2), (48, 3, 1000, 1), (20, 2, 77, 3), (64, 5, 515, 2)])
def test_f16x3_small_wavenets_vs_oracle(shape):
    c, nblk, L, B = shape
    layers = [(c, c, 2, 2 ** i) for i in range(nblk)]
    net = _cond_wavenet(c, layers, seed=c)
    g = torch.Generator().manual_seed(L)
    x, cot = torch.randn(B, c, L, generator=g), torch.randn(B, c, L, generator=g)
    _run(net, x, cot, layers, "f16x3", TOL)


def test_f16x3_mixed_widths_k3_and_dilation_beyond_length():
    layers = [(24, 40, 3, 1), (40, 40, 2, 7), (40, 72, 2, 300), (72, 72, 3, 2)]
    from wavenet_speech_amd.modules.wavenet import WaveNet
    torch.manual_seed(9)
    net = WaveNet(10, 2, layers, 36, softmax=False)
    g = torch.Generator().manual_seed(10)
    x, cot = torch.randn(2, 10, 260, generator=g), torch.randn(2, 36, 260, generator=g)
    _run(net, x, cot, layers, "f16x3", TOL)


@pytest.mark.parametrize("name", goldenio.names("wavenet_") + goldenio.names("rawctc_") + goldenio.names("classifier_"))
def test_f16x3_golden_models(name):
    """the reference's own outputs and autograd gradients (tests/golden) through the f16x3 stack, same tolerance as fp32"""
    g = goldenio.load(name)
    m = g.meta
    import wavenet_speech_amd.modules as M
    if m["kind"] == "wavenet":
        net = M.WaveNet(m["in_dim"], m["entry_kwidth"], m["layers"], m["out_dim"], softmax=m["softmax"])
    elif m["kind"] == "rawctc":
        net = M.RawCTCNet(m["num_features"], m["feature_kwidth"], m["num_labels"], m["layers"], m["out_dim"],
                          input_kernel_size=m["input_kernel_size"], input_dilation=m["input_dilation"],
                          positions=m["positions"], softmax=m["softmax"], causal=m["causal"])
    else:
        net = M.WaveNetClassifier(m["in_dim"], m["num_labels"], m["layers"], m["out_dim"],
                                  pool_kernel_size=m["pool_kernel_size"], input_kernel_size=m["input_kernel_size"],
                                  input_dilation=m["input_dilation"], softmax=m["softmax"])
    W.set_precision(net, "f16x3")
    _run_golden(g, net)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_plain_half_modes_vs_oracle(precision):
    c, L, B = 64, 600, 2
    layers = [(c, c, 2, 2 ** i) for i in range(6)]
    net = _cond_wavenet(c, layers, seed=5)
    g = torch.Generator().manual_seed(6)
    x, cot = torch.randn(B, c, L, generator=g), torch.randn(B, c, L, generator=g)
    _run(net, x, cot, layers, precision)


@pytest.mark.parametrize("precision,c,dims,L,B", [("f16x3", 256, (1, 2, 64), 384, 2), ("f16x3", 128, (1, 3), 256, 3),
                                                  ("f16x3", 256, (3, 1), 400, 2), ("f16x3", 256, (1,), 16, 1),
                                                  ("f16", 256, (1, 4), 256, 2), ("bf16", 256, (2, 1), 384, 1),
                                                  ("f16x3", 512, (1, 130), 128, 1)])
def test_full_tile_shapes_take_the_16x16x32_gemm(precision, c, dims, L, B):
    """rows a multiple of 256 (gate: channels a multiple of 128) and L a multiple of 16 select hgemm8_kernel in the f16x3 mode
    (256 x 256 tiles on v_mfma_f32_16x16x32, 32-channel k-steps, its own weight packing; L = 400 and 16 leave a partial last
    tile): all four epilogues against the oracle.  By default that is the gate and skips_sum GEMMs; test_every_gemm_and_mode_on_the_16x16x32_kernel runs the same
    cases with WN_HGEMM16=2 (every GEMM, every mode) in a child process; WN_HGEMM16=0 keeps every shape on hgemm_kernel."""
    layers = [(c, c, 2, d) for d in dims]
    net = _cond_wavenet(c, layers, seed=c + L)
    g = torch.Generator().manual_seed(L + B)
    x, cot = torch.randn(B, c, L, generator=g), torch.randn(B, c, L, generator=g)
    _run(net, x, cot, layers, precision, TOL if precision == "f16x3" else None)
    # inference (no saved tanh / sigmoid, per-block skip accumulation on the other kernel) agrees with the training forward
    net = net.to(DEV)
    with torch.no_grad():
        y_eval = net(x.to(DEV))
    y_train = net(x.to(DEV)).detach()
    assert O.rel_err(y_eval.cpu(), y_train.cpu()) < (1e-5 if precision == "f16x3" else 2e-2)


def test_f16x3_two_skips_sum_groups_on_full_tiles():
    """34 blocks = two long-K skips_sum launches (32 + 2 blocks), the second accumulating into the first's output, at a
    shape that runs on hgemm8_kernel"""
    c, L = 256, 128
    layers = [(c, c, 2, 1 + (i % 3)) for i in range(34)]
    net = _cond_wavenet(c, layers, seed=77)
    g = torch.Generator().manual_seed(78)
    x, cot = torch.randn(1, c, L, generator=g), torch.randn(1, c, L, generator=g)
    _run(net, x, cot, layers, "f16x3", TOL)


def test_every_gemm_and_mode_on_the_16x16x32_kernel():
    """by default only the f16x3 gate and skips_sum GEMMs of full-tile shapes run on hgemm8_kernel (measured: the others gain
    nothing or lose); WN_HGEMM16=2 in a child process puts every GEMM of every mode there: all epilogues, all three modes"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WN_HGEMM16="2")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_half.py"), "-q", "-x", "-k",
                        "full_tile or two_skips_sum"], env=env, cwd=root, capture_output=True, text=True)
    assert r.returncode == 0 and "8 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]


def test_half_inference_matches_training_forward_and_is_deterministic():
    c = 64
    layers = [(c, c, 2, 2 ** i) for i in range(5)]
    net = _cond_wavenet(c, layers, seed=11).to(DEV)
    W.set_precision(net, "f16x3")
    x = torch.randn(2, c, 400, device=DEV)
    y_train = net(x).detach()
    with torch.no_grad():
        y_eval = net(x)
        y_eval2 = net(x)
    assert O.rel_err(y_eval.cpu(), y_train.cpu()) < 1e-5
    assert torch.equal(y_eval, y_eval2)
    W.set_precision(net, "f32")
    with torch.no_grad():
        y32 = net(x)
    assert O.rel_err(y_eval.cpu(), y32.cpu()) < 1e-5


def test_fp16_overflow_is_loud():
    """fp16 holds the residual stream up to 16 * 65504: beyond that the call must fail, not return inf/garbage -- at once
    for an inference call, by the next call into the stack (or check_fp16_overflow()) for a training call, whose flag is
    read without stalling the stream"""
    c = 32
    layers = [(c, c, 2, 1), (c, c, 2, 2)]
    net = _cond_wavenet(c, layers, seed=13).to(DEV)
    W.set_precision(net, "f16x3")
    x = torch.randn(1, c, 100, device=DEV) * 3e6
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="overflow"):
            net(x)
    # training call: the flag travels asynchronously; whichever library call first finds it landed raises (that can be a later
    # kernel launch of the same model call -- the output-stack convs poll too), at the latest check_device_flags()
    with pytest.raises(RuntimeError, match="overflow"):
        net(x)
        W.check_fp16_overflow()
    for _ in range(4):                                   # flags of later launches of the same call may still be in flight
        try:
            W.check_fp16_overflow()
            break
        except RuntimeError:
            pass
    W.check_fp16_overflow()                              # nothing left pending
    W.set_precision(net, "bf16")
    assert bool(torch.isfinite(net(x)).all())


def test_f16x3_cfg3_one_utterance_vs_oracle():
    """the full configs[2] utterance (256 ch x 30 blocks x 16000 steps) at the fp32 path's own 1e-4 bar"""
    c, L = 256, 16000
    layers = _layers(c, 3)
    net = _wavenet(c, layers)
    x, cot = _onehot(1, c, L, 1)
    errs = _run(net, x, cot, layers, "f16x3", TOL)
    assert errs["forward"] < 2e-5


def test_f16x3_survives_the_reference_init_at_30_blocks():
    """reference init: the residual stream reaches ~7e4 and gradients grow ~2^15 on the way back -- inside the range the
    built-in power-of-two scales leave (no overflow error).  This map is ill-conditioned (two CPU fp32 summation orders
    differ by 4.5e-4 themselves); hi+lo carries 22-23 significant bits against fp32's 24, and the
    amplification multiplies that: the f16x3 result is allowed 10x the CPU fp32 path's own distance from fp64."""
    c, L = 256, 4000
    layers = _layers(c, 3)
    net = _wavenet(c, layers, seed=7, conditioned=False)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x, cot = _onehot(1, c, L, 8)
    with torch.no_grad():
        y64 = O.wavenet(x.double(), {k: v.double() for k, v in sd.items()}, layers, False, impl="taps")
        y_cpu = O.wavenet(x, sd, layers, False, impl="aten")
    net = net.to(DEV)
    W.set_precision(net, "f16x3")
    y = net(x.to(DEV))
    (y * cot.to(DEV)).sum().backward()            # must not raise
    e_cpu, e_hip = O.rel_err(y_cpu.double(), y64), O.rel_err(y.detach().cpu().double(), y64)
    print("reference init, 30 blocks: CPU fp32 vs fp64 %.2e, f16x3 vs fp64 %.2e" % (e_cpu, e_hip))
    assert e_hip < max(TOL, 10.0 * e_cpu)
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)


def test_cfg2_bf16_full_batch():
    """BASELINE configs[1] as stated: RawCTCNet 128 ch x (10 + input) blocks, L=4096, batch 32, bf16.  Size-independent
    properties at the full size plus one utterance against the oracle; the bf16 error is the storage format's (8 bits)."""
    from wavenet_speech_amd.modules.raw_ctcnet import RawCTCNet
    torch.manual_seed(12)
    layers = [(128, 128, 2, 2 ** i) for i in range(10)]
    net = RawCTCNet(128, 3, 5, layers, 128, softmax=False, causal=False).to(DEV)
    W.set_precision(net, "bf16")
    g = torch.Generator().manual_seed(13)
    x = torch.randn(32, 1, 4096, generator=g).to(DEV)
    cot = torch.randn(32, 5, 4098, generator=g).to(DEV)
    y = _properties(net, x, cot, None, 16, causal_prefix=False, additivity_tol=2e-2)
    assert tuple(y.shape) == (32, 5, 4098)
    # two utterances of the same model, forward and every gradient, against the rounding reference (tests/halfref.py)
    import copy
    small = copy.deepcopy(net).cpu()
    for p in small.parameters():
        p.grad = None
    x2, cot2 = x[6:8].cpu(), cot[6:8].cpu()
    _run(small, x2, cot2, layers, "bf16", input_grad=False, label=" cfg2 B=2 L=4096",
         kernels=lambda k: k.get("hfused_fwd_kernel", 0) > 0 and k.get("hcol2_kernel<dx+dz>", 0) > 0)


def test_cfg5_f16_full_depth_and_length():
    """BASELINE configs[4]'s shape on one GPU in its stated dtype: WaveNet 512 ch x 60 blocks x L=48000, batch 2, fp16
    (conditioned residual path: 60 random-init blocks amplify by ~2^30, beyond fp16 whatever the kernel)."""
    c, L, B = 512, 48000, 2
    layers = _layers(c, 6)
    net = _wavenet(c, layers, seed=21).to(DEV)
    W.set_precision(net, "f16")
    g = torch.Generator().manual_seed(22)
    x = torch.randn(B, c, L, generator=g).to(DEV)
    cot = torch.randn(B, c, L, generator=g).to(DEV)
    _properties(net, x, cot, 8192, 1, causal_prefix=True, additivity_tol=2e-2)


def test_cfg5_f16_full_depth_gradients_vs_rounding_reference():
    """all 60 blocks of configs[4] (512 ch, f16) on one utterance of 3000 steps: forward, dx and every parameter gradient against
    the rounding reference (tests/halfref.py)"""
    c, L = 512, 3000
    layers = _layers(c, 6)
    net = _wavenet(c, layers, seed=23)
    g = torch.Generator().manual_seed(24)
    x, cot = torch.randn(1, c, L, generator=g), torch.randn(1, c, L, generator=g)
    _run(net, x, cot, layers, "f16", label=" cfg5 60 blocks L=3000",
         kernels=lambda k: "hfused_fwd_kernel" not in k and k.get("hgemm_kernel<gate>", 0) >= 60)


def test_f16x3_wide_stack_multi_slab():
    """512 channels: eight 128-row gate slabs, four-slab block GEMMs, two-tile weight gradients"""
    c = 512
    layers = [(c, c, 2, d) for d in (1, 64, 4)]
    net = _cond_wavenet(c, layers, seed=31)
    g = torch.Generator().manual_seed(32)
    x, cot = torch.randn(1, c, 700, generator=g), torch.randn(1, c, 700, generator=g)
    _run(net, x, cot, layers, "f16x3", TOL)


def test_fp16_weight_beyond_range_is_loud():
    """weights are packed as 256 * 16 * w in the fp16 modes, so |w| >= 16 becomes inf and inf * 0 = NaN downstream; the
    store-side checks are written !(|v| <= 65504) so that the NaN trips the overflow flag instead of passing silently"""
    layers = [(32, 32, 2, 1), (32, 32, 2, 2)]
    net = _cond_wavenet(32, layers, seed=3).to(DEV)
    W.set_precision(net, "f16")
    with torch.no_grad():
        net.convolutions[0].conv_tanh.conv1d.weight[3, 5, 1] = 32.0
        with pytest.raises(RuntimeError, match="fp16 overflow"):
            net(torch.randn(1, 32, 200, device=DEV))
            W.check_device_flags()


def test_grad_scale_kernel_matches_the_torch_expression():
    from wavenet_speech_amd import functional_half as FH
    mode = FH._Mode("f16")
    for n, mag in ((1000003, 3.7), (64, 1e-12), (5, 7e9), (4096, 0.0)):
        x = torch.randn(n, device=DEV) * mag
        dyn, inv = FH._grad_scale(x, mode)
        amax = x.abs().amax().clamp_min(1e-30)
        want = torch.exp2(torch.floor(torch.log2(FH.GRAD_TARGET / amax)).clamp(-100.0, 100.0))
        assert float(dyn) == float(want), (n, mag, float(dyn), float(want))
        assert float(inv) == 1.0 / float(want)


def test_grad_scale_tail_lanes_small_counts_and_clamped_grid():
    """absmax_kernel reads 16-byte vectors and leaves n % 4 elements to the first lanes of workgroup 0; its grid is clamped to 2048
    workgroups (beyond 4 x 256 x 2048 elements a thread strides).  The maximum in the first element, in the last, in the first
    element of the tail and in the middle, at counts with every n % 4, below one vector, and past the clamp."""
    from wavenet_speech_amd import functional_half as FH
    mode = FH._Mode("f16")
    big = 4 * 256 * 2049
    assert big // 4 // 256 > 2048
    for n in (1, 2, 3, 4, 5, 6, 7, 1025, 1026, 1027, 262147, big, big + 1, big + 2, big + 3):
        for pos in sorted({0, n - 1, (n // 4) * 4 if n % 4 else n - 1, n // 2, max(n - 2, 0)}):
            x = torch.randn(n, device=DEV) * 1e-3
            x[pos] = -37.0 if pos % 2 else 37.0
            dyn, inv = FH._grad_scale(x, mode)
            amax = x.abs().amax().clamp_min(1e-30)
            assert float(amax) == 37.0
            want = torch.exp2(torch.floor(torch.log2(FH.GRAD_TARGET / amax)).clamp(-100.0, 100.0))
            assert float(dyn) == float(want) == 2.0 ** -8, (n, pos, float(dyn), float(want))
            assert float(inv) == 1.0 / float(want)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_cotangent_is_loud_in_f16(bad):
    """a NaN or inf in the cotangent of an f16 training call must not come back as finite-looking gradients.  absmax_kernel's fmaxf
    drops NaNs, so the gradient scale is that of the finite elements (inf: the smallest scale, 2^-100); the cotangent is then stored
    scaled into the fp16 series, where NaN and inf fail the store-side test !(|v| <= 65504): the fp16-overflow error is raised, at
    the latest by check_device_flags().  (Every returned gradient being non-finite would be loud as well.)"""
    c = 32
    layers = [(c, c, 2, 1), (c, c, 2, 2)]
    net = _cond_wavenet(c, layers, seed=19).to(DEV)
    W.set_precision(net, "f16")
    g = torch.Generator().manual_seed(20)
    x, cot = torch.randn(2, c, 120, generator=g).to(DEV), torch.randn(2, c, 120, generator=g)
    cot[1, 5, 77] = bad
    y = net(x)
    W.check_device_flags()
    raised = False
    try:
        y.backward(cot.to(DEV))
        W.check_device_flags()
    except RuntimeError as e:
        assert "fp16 overflow" in str(e), str(e)
        raised = True
    for _ in range(4):                                   # flags of later launches of the same call may still be in flight
        try:
            W.check_fp16_overflow()
            break
        except RuntimeError:
            pass
    W.check_fp16_overflow()                              # nothing left pending
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    print("f16 cotangent with %s: %s" % (bad, "fp16 overflow raised" if raised else "no error, %d of %d gradients non-finite"
                                         % (sum(not bool(torch.isfinite(t).all()) for t in grads), len(grads))))
    assert raised or (grads and all(not bool(torch.isfinite(t).all()) for t in grads))


# ---- plain bf16 / f16 across the half-mode dispatch, against the rounding reference (tests/halfref.py) ----------------------------

def _all_k3_on_hgemm(n):
    return lambda k: "hfused_fwd_kernel" not in k and k.get("hgemm_kernel<gate>", 0) >= n and k.get("hgemm_kernel<dz,dgate>", 0) >= n \
        and not any(n_.startswith("hcol_kernel<dz") or n_.startswith("hcol2") for n_ in k) and "hwgrad_kernel" in k


def _fused_and_hgemm(k):
    return k.get("hfused_fwd_kernel", 0) > 0 and k.get("hgemm_kernel<gate>", 0) > 0 and "hwgrad_kernel" in k


def _column_owner(k):
    return k.get("hfused_fwd_kernel", 0) > 0 and (k.get("hcol2_kernel<dx+dz>", 0) > 0 or k.get("hcol_kernel<dz,dgate>", 0) > 0)


def _notebook_layers(c):
    """the reference's training model (RawCTCNet on Gaussian Model (Train), cell 5): 21 blocks of k=2 then 21 of k=3"""
    dil = [1, 2, 4, 8, 16, 32, 64] * 3
    return [(c, c, 2, d) for d in dil] + [(c, c, 3, d) for d in dil]


WAVENET_CASES = {  # layers, skip rows, B, L, kernels
    "k3_32_short_utts_d_ge_L": ([(32, 32, 3, 1), (32, 32, 3, 8)], 32, 6, 5, _all_k3_on_hgemm(2)),
    "k3_64_ragged": ([(64, 64, 3, d) for d in (1, 2, 4)], 64, 2, 301, _all_k3_on_hgemm(3)),
    "k3_128_d_ge_L": ([(128, 128, 3, d) for d in (1, 200)], 128, 2, 150, _all_k3_on_hgemm(2)),
    "k3_256_skip128": ([(256, 256, 3, d) for d in (1, 4)], 128, 2, 257, _all_k3_on_hgemm(2)),
    "k3_512_skip256": ([(512, 512, 3, d) for d in (2, 1)], 256, 1, 300, _all_k3_on_hgemm(2)),
    "k3_256_short_utts_d_ge_L": ([(256, 256, 3, 1), (256, 256, 3, 16)], 128, 5, 9, _all_k3_on_hgemm(2)),
    "k3_512_d_ge_L_ragged": ([(512, 512, 3, d) for d in (300, 2)], 512, 2, 130, _all_k3_on_hgemm(2)),
    "mixed_k_alternating_64": ([(64, 64, 2 + (i % 2), 2 ** (i % 5)) for i in range(12)], 64, 2, 130, _fused_and_hgemm),
    "mixed_widths_64_256_64": ([(64, 64, 2, 1), (64, 256, 3, 2), (256, 256, 2, 4), (256, 64, 2, 1), (64, 64, 2, 8)], 64, 2, 200,
                               _fused_and_hgemm),
    "narrow_under_wide": ([(64, 64, 2, 1), (64, 256, 2, 2)] + [(256, 256, 2, 2 ** i) for i in range(2, 8)], 64, 1, 160,
                          _fused_and_hgemm),
    # (a skip path wider than the blocks keeps dz / dx on the tiled kernels)
    "chain_96_skip128": ([(96, 96, 2, d) for d in (1, 2, 4)], 128, 2, 300,
                         lambda k: k.get("hfused_fwd_kernel", 0) > 0 and k.get("hgemm_kernel<dz,dgate>", 0) >= 3),
    "chain_128": ([(128, 128, 2, d) for d in (1, 2, 4, 8)], 128, 2, 300, _column_owner),
    "one_time_step": ([(128, 128, 2, 1), (128, 128, 2, 2)], 128, 1, 1, _column_owner),
    "more_utts_than_unit_columns": ([(64, 64, 2, d) for d in (1, 2)], 64, 40, 3, _column_owner),
}


@pytest.mark.parametrize("precision", PLAIN)
@pytest.mark.parametrize("case", sorted(WAVENET_CASES))
def test_plain_half_wavenet_dispatch_vs_rounding_reference(precision, case):
    layers, ms, B, L, kernels = WAVENET_CASES[case]
    net = _cond_wavenet(layers[0][0], layers, seed=len(case), out_dim=ms)
    g = torch.Generator().manual_seed(B * L)
    x, cot = torch.randn(B, layers[0][0], L, generator=g), torch.randn(B, ms, L, generator=g)
    _run(net, x, cot, layers, precision, kernels=kernels, label=" " + case)


@pytest.mark.parametrize("case", sorted(WAVENET_CASES))
def test_f16x3_wavenet_dispatch_vs_oracle(case):
    """the same shapes in f16x3, which takes neither the fused forward nor the column-owner kernels: the fp32 path's 1e-4 bar"""
    layers, ms, B, L, _ = WAVENET_CASES[case]
    net = _cond_wavenet(layers[0][0], layers, seed=len(case), out_dim=ms)
    g = torch.Generator().manual_seed(B * L)
    x, cot = torch.randn(B, layers[0][0], L, generator=g), torch.randn(B, ms, L, generator=g)
    _run(net, x, cot, layers, "f16x3", TOL, label=" " + case,
         kernels=lambda k: "hfused_fwd_kernel" not in k and not any(n.startswith("hcol") for n in k)
         and k.get("hgemm_kernel<dz,dgate>", 0) >= len(layers) and "hwgrad_kernel" in k)


RAWCTC_CASES = {  # channels, layers, causal, feature kwidth, skip rows, B, L, kernels
    "k3_64_noncausal": (64, [(64, 64, 3, d) for d in (1, 2, 5)], False, 3, 64, 2, 300, _fused_and_hgemm),
    "k3_256_noncausal_skip128": (256, [(256, 256, 3, d) for d in (1, 3)], False, 3, 128, 1, 200, _all_k3_on_hgemm(3)),
    "notebook_64": (64, _notebook_layers(64), True, 1, 64, 2, 117, _fused_and_hgemm),
    "notebook_128": (128, _notebook_layers(128), True, 1, 128, 2, 117, _fused_and_hgemm),
}


@pytest.mark.parametrize("precision", PLAIN)
@pytest.mark.parametrize("case", sorted(RAWCTC_CASES))
def test_plain_half_rawctcnet_dispatch_vs_rounding_reference(precision, case):
    """RawCTCNet: feature layer and output block inside the stack function; non-causal taps (offsets -d, 0, +d); the notebook's
    mixed k=2 / k=3 stack, whose weight-gradient groups could not be planned before they were formed per block"""
    c, layers, causal, kf, ms, B, L, kernels = RAWCTC_CASES[case]
    net = _cond_rawctc(c, layers, causal, seed=c + len(layers), feature_kwidth=kf, out_dim=ms)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, 1, L, generator=g)
    cot = torch.randn(B, 5, L + kf - 1, generator=g)
    _run(net, x, cot, layers, precision, input_grad=False, kernels=kernels, label=" " + case)


@pytest.mark.parametrize("precision", PLAIN)
def test_reference_training_model_in_half_modes(precision):
    """the reference's own training model (RawCTCNet 512 ch, 21 blocks k=2 + 21 blocks k=3 at dilations 1..64, causal,
    feature_kwidth=1, batch 8, raw one-channel signal of 117 samples) in a plain half mode, with a conditioned residual path"""
    layers = _notebook_layers(512)
    net = _cond_rawctc(512, layers, True, seed=117, feature_kwidth=1)
    g = torch.Generator().manual_seed(118)
    x, cot = torch.randn(8, 1, 117, generator=g), torch.randn(8, 5, 117, generator=g)
    _run(net, x, cot, layers, precision, input_grad=False, label=" reference model 512ch x 43",
         kernels=lambda k: k.get("hgemm_kernel<gate>", 0) >= 43)


@pytest.mark.parametrize("precision", PLAIN)
def test_frozen_entry_conv_needs_no_input_gradient(precision):
    """the stack's input needs no gradient (entry conv frozen, data without gradient) at the bottom of a paired chain: the
    bottom block's dz is all backward needs from it"""
    c = 64
    layers = [(c, c, 2, d) for d in (1, 2, 4)]
    net = _cond_wavenet(c, layers, seed=66)
    for p in net.entry_conv1d.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(67)
    x, cot = torch.randn(2, c, 250, generator=g), torch.randn(2, c, 250, generator=g)
    _run(net, x, cot, layers, precision, input_grad=False, kernels=_column_owner, label=" frozen entry conv")


def test_negative_leaky_slope_is_not_fused():
    """the series kernels take the sign of the stored activation as the LeakyReLU backward mask, valid for slopes >= 0 only: a
    model with a negative slope runs its feature layer and output block outside the stack function"""
    from wavenet_speech_amd.modules.block import fusable_front, fusable_head
    layers = [(64, 64, 2, d) for d in (1, 2, 4)]
    net = _cond_rawctc(64, layers, False, seed=5, slope=-0.2)
    assert fusable_head(net.output_block, "bf16") is None
    assert fusable_front(net.feature_layer, "bf16", torch.zeros(1, 1, 8)) is None
    g = torch.Generator().manual_seed(6)
    x, cot = torch.randn(2, 1, 300, generator=g), torch.randn(2, 5, 302, generator=g)
    _run(net, x, cot, layers, "bf16", input_grad=False, label=" negative slope")


def test_predicate_rejects_plausible_kernel_bugs():
    """the predicate has teeth: references built from slightly altered parameters -- each what a plausible kernel bug would
    compute -- are rejected for the unaltered GPU result (only the reference side changes)"""
    c = 128
    layers = [(c, c, 2, 1), (c, c, 3, 2), (c, c, 2, 4), (c, c, 2, 8)]
    net = _cond_wavenet(c, layers, seed=41)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(42)
    x, cot = torch.randn(2, c, 500, generator=g), torch.randn(2, c, 500, generator=g)

    def altered(key, f):
        s = dict(sd)
        s[key] = f(s[key].clone())
        return s, None

    def last_tap(w):
        w[:, :, -1] *= 1 + 2 ** -5
        return w
    off_by_one = list(layers)
    off_by_one[2] = (c, c, 2, 5)
    mutants = {
        "conv_sigmoid bias of block 1 zero": altered("convolutions.1.conv_sigmoid.conv1d.bias", torch.zeros_like),
        "last conv_tanh tap of block 1 x (1 + 2^-5)": altered("convolutions.1.conv_tanh.conv1d.weight", last_tap),
        "residual_proj bias of block 2 dropped": altered("convolutions.2.residual_proj.bias", torch.zeros_like),
        "dilation of block 2 off by one": (dict(sd), off_by_one),
    }
    _run(net, x, cot, layers, "bf16", kernels=_fused_and_hgemm, label=" mutant base", mutants=mutants)
