#!/usr/bin/env python3
"""Time the per-base qualities (csrc/wn_quality.hip through wavenet_speech_amd.decoding.ctc_base_qualities) on the GPU next to
the greedy decode of the SAME logits, which reads the same bytes once: peaked [B, C, T] logits (a random path of runs with
dwells 1-12, as a trained model's output looks), C = 5, for B in {8, 32}, T in {4096, 100000}, stat "mean".  Reports min /
median / max ms per call (device events around every one of `reps` calls after `warmup` calls), the number of bases, and the
ratio of the medians.  The quality call is what a user calls: two launches and the few torch ops on [B] tensors around them.
Writes its table to --out, by default profiles/rNN/quality_bench.txt in the next free rNN.
Usage: quality_bench.py [--reps N] [--warmup N] [--quick] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet_speech_amd import decoding as D  # noqa: E402

from gputime import Report, next_profile_dir, timed  # noqa: E402


def gpu_ms(fn, reps, warmup):
    """(min, median, max) ms of one call"""
    return timed(fn, windows=reps, warmup=warmup)[:3]


def peaked_logits(seed, B, C, T, margin=6.0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, C, T)).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            c, d = int(rng.integers(0, C)), int(rng.integers(1, 13))
            x[b, c, t:t + d] += margin * rng.uniform(0.6, 1.0)
            t += d
    return torch.from_numpy(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="B=8, T=4096 only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quality_bench.py measures the GPU; there is no CPU path"
    C = 5
    Bs, Ts = ([8], [4096]) if a.quick else ([8, 32], [4096, 100000])
    rep = Report()
    lines = ["# per-base qualities next to the greedy decode of the same logits, C=%d, fp32 [B][C][T], %s; reps=%d warmup=%d; "
             "ms per call: min / median / max" % (C, torch.cuda.get_device_name(0), a.reps, a.warmup),
             "%4s %7s %9s %26s %26s %7s" % ("B", "T", "bases", "greedy decode ms", "base qualities ms", "ratio")]
    for line in lines:
        rep.emit(line)
    for B in Bs:
        for T in Ts:
            x = peaked_logits(B * 1000003 + T, B, C, T).to("cuda:0")
            labels, lengths, frames = D.ctc_greedy_decode(x)
            g = gpu_ms(lambda: D.ctc_greedy_decode(x), a.reps, a.warmup)
            q = gpu_ms(lambda: D.ctc_base_qualities(x, labels, lengths, frames), a.reps, a.warmup)
            line = "%4d %7d %9d %26s %26s %7.2f" % (B, T, int(lengths.sum()), "%.3f / %.3f / %.3f" % g, "%.3f / %.3f / %.3f" % q,
                                                    q[1] / g[1])
            rep.emit(line)
    torch.cuda.synchronize()
    from wavenet_speech_amd import check_device_flags
    check_device_flags()
    out = a.out or os.path.join(next_profile_dir(), "quality_bench.txt")
    rep.save(out)
    print("wrote", out)


if __name__ == "__main__":
    main()
