#!/usr/bin/env python3
"""Time the quality profile (csrc/wn_profile.hip through wavenet_speech_amd.decoding.quality_profile) on the GPU next to the
pairwise_align call that produced its input: B in {8, 32} pairs of about 400 labels (a truth and a copy with 6 % substitutions,
insertions and deletions each), one pair of 8192 x 8192 labels made the same way, and one pair of 8192 x 8192 labels over
disjoint alphabets, whose end-gap-free alignment is all gaps: the full 16 384 columns (profiled with count_ends=True, so that
every column is tabulated).  qual and dwell are random.  Reports min / median / max ms per call (device events around every one
of `reps` calls after `warmup` calls), the columns walked, and the ratio of the medians.  Both calls are what a user calls: the
launch and the allocations, the zeroed flag and its asynchronous read-back around it.
Writes its table to --out, by default profiles/rNN/profile_bench.txt in the next free rNN.
Usage: profile_bench.py [--reps N] [--warmup N] [--quick] [--out FILE]"""
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


def pairs(seed, B, n_lo, n_hi, width, rate=0.06, unrelated=False):
    """(truth [B, width], lengths, calls [B, width], lengths) as int32 arrays: labels 1..4"""
    rng = np.random.default_rng(seed)
    truth, calls = np.zeros((B, width), np.int32), np.zeros((B, width), np.int32)
    tn, cn = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        t = rng.integers(1, 5, size=int(rng.integers(n_lo, n_hi + 1)))
        if unrelated:
            t, q = np.full(width, 1), np.full(width, 2)
        else:
            u = rng.random(len(t))
            sub = np.where(u < rate, 1 + (t + rng.integers(0, 3, size=len(t))) % 4, t)
            keep = ~((u >= rate) & (u < 2 * rate))
            ins = rng.random(len(t)) < rate
            q = []
            for v, k, i in zip(sub.tolist(), keep.tolist(), ins.tolist()):
                if k:
                    q.append(v)
                if i:
                    q.append(int(rng.integers(1, 5)))
            q = np.asarray(q[:width])
        truth[b, :len(t)], calls[b, :len(q)], tn[b], cn[b] = t, q, len(t), len(q)
    return truth, tn, calls, cn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="B=8 pairs of about 400 labels only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "profile_bench.py measures the GPU; there is no CPU path"
    dev = "cuda:0"
    work = [("8 x ~400", 8, 350, 450, 512, False, False), ("32 x ~400", 32, 350, 450, 512, False, False),
            ("1 x 8192 mutated", 1, 7600, 7600, 8192, False, False), ("1 x 8192 16384 col", 1, 8192, 8192, 8192, True, True)]
    if a.quick:
        work = work[:1]
    rep = Report()
    lines = ["# quality profile next to the pairwise alignment that made its ops, classes=5, qual and dwell given, %s; reps=%d "
             "warmup=%d; ms per call: min / median / max" % (torch.cuda.get_device_name(0), a.reps, a.warmup),
             "%-19s %8s %26s %26s %7s" % ("pairs", "columns", "pairwise_align ms", "quality_profile ms", "ratio")]
    for line in lines:
        rep.emit(line)
    for n, (name, B, lo, hi, width, unrelated, count_ends) in enumerate(work):
        truth, tn, calls, cn = (torch.from_numpy(v).to(dev) for v in pairs(1000 + n, B, lo, hi, width, unrelated=unrelated))
        g = torch.Generator().manual_seed(n)
        qual = torch.randint(0, 94, calls.shape, generator=g, dtype=torch.uint8).to(dev)
        dwell = torch.randint(1, 40, calls.shape, generator=g, dtype=torch.int32).to(dev)
        al = D.pairwise_align(truth, tn, calls, cn)
        prof = D.quality_profile(al, truth, tn, calls, cn, qual=qual, dwell=dwell, count_ends=count_ends)
        assert int(prof.read_counts.sum()) == int(al.ops_len.sum())
        t_al = gpu_ms(lambda: D.pairwise_align(truth, tn, calls, cn), a.reps, a.warmup)
        t_pr = gpu_ms(lambda: D.quality_profile(al, truth, tn, calls, cn, qual=qual, dwell=dwell, count_ends=count_ends), a.reps, a.warmup)
        line = "%-19s %8d %26s %26s %7.3f" % (name, int(al.ops_len.sum()), "%.3f / %.3f / %.3f" % t_al, "%.3f / %.3f / %.3f" % t_pr,
                                              t_pr[1] / t_al[1])
        rep.emit(line)
    torch.cuda.synchronize()
    from wavenet_speech_amd import check_device_flags
    check_device_flags()
    out = a.out or os.path.join(next_profile_dir(), "profile_bench.txt")
    rep.save(out)
    print("wrote", out)


if __name__ == "__main__":
    main()
