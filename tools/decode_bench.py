#!/usr/bin/env python3
"""Time the CTC decoders (csrc/wn_decode.hip through wavenet_speech_amd.decoding) on the GPU: greedy and prefix beam search on
random [B, C, T] logits, C = 5, for B in {8, 32}, T in {1024, 4096}, W in {1, 8, 32, 64}.  Reports ms per batch (device
events around `reps` calls after `warmup` calls) and us per frame-step (ms per batch / T: the utterances of a batch run in
parallel, so a step of the beam recursion costs that much wall time).  With --cpu-ref also the plain-Python CPU reference of
the tests (tests/ctc_decode_ref.py), timed on ONE utterance per shape and multiplied by B (it decodes utterances one after
another).  Usage: decode_bench.py [--reps N] [--warmup N] [--cpu-ref] [--quick] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from wavenet_speech_amd import decoding as D  # noqa: E402

from gputime import Report, timed  # noqa: E402


def gpu_ms(fn, reps, warmup):
    return timed(fn, calls=reps, warmup=warmup).median


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--quick", action="store_true", help="B=8, T=1024 only (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decode_bench.py measures the GPU; there is no CPU path"
    C = 5
    Bs, Ts, Ws = ([8], [1024], [1, 8, 32, 64]) if a.quick else ([8, 32], [1024, 4096], [1, 8, 32, 64])
    lines = ["# CTC decoding, C=%d, fp32 logits [B][C][T], %s; reps=%d warmup=%d" % (C, torch.cuda.get_device_name(0), a.reps, a.warmup),
             "%-7s %4s %5s %3s %12s %14s %16s" % ("decoder", "B", "T", "W", "gpu ms/batch", "gpu us/step", "cpu-ref ms/batch")]
    rep = Report()
    emit = rep.emit
    for line in lines:
        emit(line)
    ref_cache = {}
    for B in Bs:
        for T in Ts:
            g = torch.Generator().manual_seed(B * 100000 + T)
            xh = torch.randn(B, C, T, generator=g) * 1.5
            x = xh.to("cuda:0")
            ms = gpu_ms(lambda: D.ctc_greedy_decode(x), a.reps, a.warmup)
            cpu = ""
            if a.cpu_ref:
                from tests import ctc_decode_ref as R
                t = time.perf_counter()
                R.greedy_decode_batch(xh.numpy())
                cpu = "%.1f" % ((time.perf_counter() - t) * 1e3)
            emit("%-7s %4d %5d %3s %12.3f %14.3f %16s" % ("greedy", B, T, "-", ms, ms * 1e3 / T, cpu))
            for W in Ws:
                ms = gpu_ms(lambda: D.ctc_beam_decode(x, W), a.reps, a.warmup)
                cpu = ""
                if a.cpu_ref:
                    from tests import ctc_decode_ref as R
                    if (T, W) not in ref_cache:
                        t = time.perf_counter()
                        R.beam_decode(xh[0].numpy(), W)
                        ref_cache[(T, W)] = time.perf_counter() - t
                    cpu = "%.0f (1 utt x %d)" % (ref_cache[(T, W)] * 1e3 * B, B)
                emit("%-7s %4d %5d %3d %12.3f %14.3f %16s" % ("beam", B, T, W, ms, ms * 1e3 / T, cpu))
    torch.cuda.synchronize()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
