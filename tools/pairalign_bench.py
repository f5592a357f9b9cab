#!/usr/bin/env python3
"""Time pairwise alignment (csrc/wn_pairalign.hip through wavenet_speech_amd.pairwise_align / edit_distance) on the GPU:
B in {8, 32} pairs of about 400 labels -- the reads of a 4096-frame utterance: a random reference and a query made from it by
15 % substitutions, insertions and deletions -- and one pair of 8192 x 8192, with needle's costs and free end gaps.  Reports
ms per batch for the full form (score, counts, ops), the score-only form (edit_distance: the fill alone, so the difference is
the backpointer stores and the trace) and cells per microsecond; device events around `reps` calls after `warmup` calls,
output buffers allocated inside the Python call.  In the same run it times the beam decode (W = 8) of B = 32 utterances of
T = 4096 frames, the step that produces such reads: aligning a batch should cost less than decoding it.
With --cpu-ref also the numpy reference of the tests (tests/pairwise_align_ref.py) on ONE pair per shape.
Usage: pairalign_bench.py [--reps N] [--warmup N] [--cpu-ref] [--quick] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet_speech_amd import _lib  # noqa: E402
from wavenet_speech_amd import decoding as D  # noqa: E402

from gputime import Report, timed  # noqa: E402


def gpu_ms(fn, reps, warmup):
    return timed(fn, calls=reps, warmup=warmup).median


def mutate(rng, ref, rate):
    out = []
    for v in ref:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(int(rng.integers(1, 5)))
        if u > 1 - rate / 3:
            v = int(rng.integers(1, 5))
        out.append(int(v))
    return out


def make_pairs(B, n, seed):
    rng = np.random.default_rng(seed)
    refs = [rng.integers(1, 5, size=n).tolist() for _ in range(B)]
    queries = [mutate(rng, r, 0.15)[:n] for r in refs]
    a = np.zeros((B, n), dtype=np.int32)
    b = np.zeros((B, n), dtype=np.int32)
    for k in range(B):
        a[k, :len(refs[k])] = refs[k]
        b[k, :len(queries[k])] = queries[k]
    dev = "cuda:0"
    return (torch.tensor(a, device=dev), torch.tensor([len(r) for r in refs], dtype=torch.int32, device=dev),
            torch.tensor(b, device=dev), torch.tensor([len(q) for q in queries], dtype=torch.int32, device=dev), refs, queries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--quick", action="store_true", help="B=8 pairs of 400 labels only (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "pairalign_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pairalign_bench.py measures the GPU; there is no CPU path"
    lib = _lib.load()
    shapes = [(8, 400)] if a.quick else [(8, 400), (32, 400), (1, 8192)]
    rep = Report()
    lines = ["# pairwise alignment, needle's costs, free end gaps, int32 labels, %s; reps=%d warmup=%d"
             % (torch.cuda.get_device_name(0), a.reps, a.warmup),
             "%4s %6s %6s %14s %18s %13s %12s %8s %15s" % ("B", "N", "M", "align ms/batch", "score-only ms/batch", "cells/us full",
                                                         "mean identity", "ws MB", "cpu-ref ms/pair")]
    for line in lines:
        rep.emit(line)
    for B, n in shapes:
        ref, rl, query, ql, refs, queries = make_pairs(B, n, 1000 * B + n)
        ms_full = gpu_ms(lambda: D.pairwise_align(ref, rl, query, ql), a.reps, a.warmup)
        ms_score = gpu_ms(lambda: D.edit_distance(ref, rl, query, ql), a.reps, a.warmup)
        out = D.pairwise_align(ref, rl, query, ql)
        torch.cuda.synchronize()
        cells = float((rl.double() * ql.double()).sum())
        cpu = ""
        if a.cpu_ref:
            from tests import pairwise_align_ref as R
            t = time.perf_counter()
            want = R.align(refs[0], queries[0])
            cpu = "%.0f" % ((time.perf_counter() - t) * 1e3)
            assert want.score == int(float(out.score[0]) * 2) and want.length == int(out.length[0])
        rep.emit("%4d %6d %6d %14.3f %18.3f %13.1f %12.3f %8.1f %15s" % (
            B, n, n, ms_full, ms_score, cells / (ms_full * 1e3), float(out.identity.mean()),
            lib.wn_pair_align_workspace_bytes(B, n, n) / 2**20, cpu))
    if not a.quick:
        B, C, T, W = 32, 5, 4096, 8
        g = torch.Generator().manual_seed(7)
        x = (torch.randn(B, C, T, generator=g) * 1.5).to("cuda:0")
        ms_beam = gpu_ms(lambda: D.ctc_beam_decode(x, W), a.reps, a.warmup)
        labels, lengths, _, _ = D.ctc_beam_decode(x, W)
        best, n_best = labels[:, 0], lengths[:, 0]                   # the decoder's output, aligned in place against another beam
        ms_reads = gpu_ms(lambda: D.pairwise_align(labels[:, 1], lengths[:, 1], best, n_best), a.reps, a.warmup)
        rep.emit("# beam decode W=%d of B=%d, T=%d random logits: %.3f ms/batch; aligning its best beam (mean %.0f labels, rows of %d) "
                 "against its second: %.3f ms/batch" % (W, B, T, ms_beam, float(n_best.float().mean()), T, ms_reads))
    from wavenet_speech_amd import check_device_flags
    check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
