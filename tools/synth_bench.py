#!/usr/bin/env python3
"""Time the HIP read generator (csrc/wn_synth.hip) against the same stages as torch ops on the GPU.
Usage: synth_bench.py [batch length]
       synth_bench.py --ragged [--out FILE]     the ragged generator (csrc/wn_reads.hip, two launches) next to the fixed
                                                three-launch generator at the same sample count and the torch-op form"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from wavenet_speech_amd import synthetic as S  # noqa: E402

import gputime  # noqa: E402


def ragged(out_path):
    """device events; B = 32 reads of about 700 bases, uniform (6, 2) (about cfg2's 4096 samples), and B = 16 at about 16 000"""
    def timed_ev(fn, n=50):
        return gputime.timed(fn, calls=n, warmup=5).median

    dev = "cuda:0"
    rep = gputime.Report()
    rep.emit("ragged generator, uniform dwell (6, 2), loader window; ms per call by device events, host launch overhead included")
    table = S.standin_kmer_table(device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    host_gen = torch.Generator().manual_seed(1)                        # the seed is drawn on the host: no device read
    for B, nb in ((32, 700), (16, 2700)):
        lo, hi = nb - 8, nb + 8
        pad = (hi - 9) * 7                                              # no read can be longer
        plan = S.hip_reads_plan(B, lo, hi, 2, ("uniform", 6, 2), 7, 3, dev)
        t_plan = timed_ev(lambda: S.hip_reads_plan(B, lo, hi, 2, ("uniform", 6, 2), 7, 3, dev))
        t_sig = timed_ev(lambda: S.hip_reads_signal(plan, pad, table, 3))
        t_both = timed_ev(lambda: S.ragged_reads(B, (lo, hi), ("uniform", 6, 2), table=table, generator=host_gen, device=dev, pad_to=pad))
        t_sync = timed_ev(lambda: S.ragged_reads(B, (lo, hi), ("uniform", 6, 2), table=table, generator=host_gen, device=dev))
        samples = int(plan["signal_lengths"].max())
        fixed_bases = S.hip_bases(B, -(-samples // 3) + 8, 11, dev)

        def fixed():
            S.hip_bases(B, -(-samples // 3) + 8, 11, dev)
            S.hip_signal(fixed_bases, samples, 256, 3, table, seed=3, want_one_hot=False)
        t_fixed = timed_ev(fixed)
        t_torch = timed_ev(lambda: S._torch_reads(B, lo, hi, 2, ("uniform", 6, 2), 7, table, gen, torch.device(dev), pad, None, None, None,
                                                  None), n=20)
        for line in ("B = %d, %d..%d bases, longest read %d samples, rows of %d" % (B, lo, hi - 1, samples, pad),
                     "  wn_reads_plan                          : %.3f ms" % t_plan,
                     "  wn_reads_signal                        : %.3f ms" % t_sig,
                     "  ragged_reads, pad_to (two launches)    : %.3f ms" % t_both,
                     "  ragged_reads, one host read of the max : %.3f ms" % t_sync,
                     "  fixed generator, %d samples, 3 launches (bases, signal, quantize; no one-hot): %.3f ms" % (samples, t_fixed),
                     "  torch ops on the GPU (randint, cumsum, searchsorted, gather, randn)         : %.3f ms" % t_torch,
                     "  expectation (plan + signal <= fixed three-launch generator): %s" % ("holds" if t_plan + t_sig <= t_fixed else "DOES NOT HOLD")):
            rep.emit(line)
    rep.save(out_path)


if "--ragged" in sys.argv:
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r06", "ragged_bench.txt")
    ragged(out)
    sys.exit(0)

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
L = int(sys.argv[2]) if len(sys.argv) > 2 else 16000
dev = "cuda:0"


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


g = torch.Generator(device=dev).manual_seed(1)
bases = S.hip_bases(B, -(-L // 3) + 8, 11, dev)
full = timed(lambda: S.hip_signal(bases, L, 256, 3, None, seed=3))
lean = timed(lambda: S.hip_signal(bases, L, 256, 3, None, seed=3, want_one_hot=False))


def torch_ops():
    kmers = S.kmer_indices(bases, 3)[:, :L]
    means, stdvs = S.standin_kmer_table(device=dev)
    pico = S.gaussian_picoamps(kmers, (means.double(), stdvs.double()), g)
    lv = S.quantize(pico, 256)
    return S.one_hot(lv, 256)


ref = timed(torch_ops)
onehot_bytes = B * 256 * L * 4
print("generator %d x %d, 256 levels, upsampling 3 (ms per call incl. host launch overhead)" % (B, L))
print("  HIP, levels + dense one-hot : %.3f ms  (%.0f GB/s of one-hot stores)" % (full, onehot_bytes / full / 1e6))
print("  HIP, levels only            : %.3f ms" % lean)
print("  torch ops on the GPU        : %.3f ms" % ref)
