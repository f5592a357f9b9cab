#!/usr/bin/env python3
"""Time wn_hblock_forward (training form: z, sg, r stored) at BASELINE configs[1]'s block shape, fused vs two launches.
usage: fused_bench.py [C] [L] [B] [d]   (env WN_FUSED_FWD=0 for the two-launch path)
WN_LIB=libwavenet_amd_measure.so (`make -C wavenet_speech_amd/csrc measure`; as tools/run_bench_with_lib.py takes it) loads the
measurement build, which WN_FUSED_DBG=bits (ablations) and WN_FUSED_STAMPS=1 (phase stamps of wave 0 of every workgroup) need: the
product library does not read them."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wavenet_speech_amd import _lib
if os.environ.get("WN_LIB"):
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.__file__), os.environ["WN_LIB"])
from wavenet_speech_amd import functional as HF
from wavenet_speech_amd import functional_half as FH
from gputime import timed

C = int(sys.argv[1]) if len(sys.argv) > 1 else 128
L = int(sys.argv[2]) if len(sys.argv) > 2 else 4098
B = int(sys.argv[3]) if len(sys.argv) > 3 else 32
d = int(sys.argv[4]) if len(sys.argv) > 4 else 16
prec = os.environ.get("PREC", "bf16")
dev = torch.device("cuda:0")
lib = _lib.load()
mode = FH._Mode(prec)
spec = HF.BlockSpec(C, C, C, 2, d, False)
layout = FH.HalfLayout(L, spec.reach())
shape = FH._shape(spec, B, layout)
torch.manual_seed(0)
prm = [torch.randn(C, C, 2, device=dev) * 0.05, torch.randn(C, device=dev) * 0.1, torch.randn(C, C, 2, device=dev) * 0.05,
       torch.randn(C, device=dev) * 0.1, torch.randn(C, C, device=dev) * 0.05, torch.randn(C, device=dev) * 0.1,
       torch.randn(C, C, device=dev) * 0.05, torch.randn(C, device=dev) * 0.1, torch.randn(C, C, device=dev) * 0.05,
       torch.randn(C, device=dev) * 0.1]
nbytes = lib.wn_hblock_packed_bytes(ctypes.byref(shape), mode.code)
packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
ps = HF._params_struct(prm)
_lib.check(lib.wn_hblock_pack(ctypes.byref(shape), mode.code, ctypes.byref(ps), HF._p(packed), HF._stream()), "pack")
x = FH._hlease(mode, B, C, layout, dev)
FH._load(lib, mode, torch.randn(B, C, L, device=dev), x, layout, float(lib.wn_hseries_residual_scale()), None, None)
r, sg, z = (FH._hlease(mode, B, C, layout, dev) for _ in range(3))

stamps = None
if os.environ.get("WN_FUSED_STAMPS"):
    # 8 words per workgroup of the launch (csrc/wn_fused.hip: units of 32 columns, four per workgroup, the grid a multiple of 8);
    # the library writes into the caller's buffer and copies nothing back
    nwg = (-(-(B * -(-L // 32)) // 4) + 7) // 8 * 8
    stamps = torch.zeros(nwg, 8, dtype=torch.int64, device=dev)
    ctypes.CDLL(_lib.LIB_PATH).wn_debug_set_fused_stamp_buffer(ctypes.c_void_p(stamps.data_ptr()))

def run():
    _lib.check(lib.wn_hblock_forward(ctypes.byref(shape), mode.code, HF._p(packed), HF._p(x), HF._p(r), None, 0, HF._p(sg), HF._p(z),
                                     None, HF._stream()), "fwd")
us = timed(run, calls=200, warmup=20).median * 1e3
mb = B * L * C * 2 * 4 / 1e6
print("C %d L %d B %d d %d %s fused=%s dbg=%s: %.1f us per block forward  (%.0f MB algorithmic -> %.2f TB/s)" % (
    C, L, B, d, prec, os.environ.get("WN_FUSED_FWD", "1"), os.environ.get("WN_FUSED_DBG", "0"), us, mb, mb / us * 1e-6 * 1e6 / 1e6))
if stamps is not None:
    import numpy as np
    torch.cuda.synchronize()
    a = stamps.cpu().numpy()
    a = a[a[:, 7] > 0]
    d = np.diff(a, axis=1)
    names = ["gate half 0 K loop", "gate 0 epilogue", "gate 1 (K loop + epilogue)", "res K loop", "res epilogue", "-", "drain"]
    print("%d workgroups; wave 0 lifetime %.0f cycles (s_memtime ticks, 100 MHz? see below)" % (len(a), (a[:, 7] - a[:, 0]).mean()))
    for i, nm in enumerate(names):
        print("  %-24s mean %8.0f  median %8.0f" % (nm, d[:, i].mean(), np.median(d[:, i])))
    span = a[:, 7].max() - a[:, 0].min()
    print("  kernel span %d ticks; first start spread %d; starts in second half of span: %d" % (span, a[:, 0].max() - a[:, 0].min(), (a[:, 0] > a[:, 0].min() + span // 2).sum()))
