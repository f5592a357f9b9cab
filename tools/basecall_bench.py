#!/usr/bin/env python3
"""Time chunked whole-read basecalling (wavenet_speech_amd.Basecaller, csrc/wn_chunk.hip) on the GPU with BASELINE configs[1]'s
RawCTCNet (128 ch, input block + 10 blocks of dilation 1..512, feature conv k=3, bf16), chunk = 4096, batch = 32, on a set of
ragged reads (int16 DAC counts with per-read scale / shift).  Reports
  * kept samples per second of Basecaller.__call__ (host clock around calls that end in a synchronise) with graph off and on;
  * the device time of one gather and of one stitch launch per micro-batch (device events);
  * the device time of the bare no-grad model(x) on the same [batch, 1, chunk] tensor on the same build: the yardstick.
Usage: basecall_bench.py [--reads N] [--min-len N] [--max-len N] [--reps N] [--warmup N] [--precision P] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import wavenet_speech_amd as W  # noqa: E402
from wavenet_speech_amd import basecalling as BC  # noqa: E402

from gputime import Report, timed  # noqa: E402


def gpu_ms(fn, reps, warmup):
    return timed(fn, calls=reps, warmup=warmup).median


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return min(times), sorted(times)[len(times) // 2], max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=48)
    ap.add_argument("--min-len", type=int, default=20000)
    ap.add_argument("--max-len", type=int, default=120000)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--precision", default="bf16", choices=["f32", "f16x3", "f16", "bf16"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "basecall_bench.py measures the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    C = a.channels
    layers = [(C, C, 2, 2 ** i) for i in range(10)]
    net = W.RawCTCNet(C, 3, 5, layers, C, softmax=False, causal=False).to(dev)
    W.set_precision(net, a.precision)
    g = torch.Generator().manual_seed(1)
    lengths = torch.randint(a.min_len, a.max_len + 1, (a.reads,), generator=g)
    raw = torch.randint(300, 700, (a.reads, int(lengths.max())), generator=g).to(torch.int16).to(dev)
    scale = torch.full((a.reads,), 1.0 / 60.0, device=dev)
    shift = torch.full((a.reads,), -500.0, device=dev)
    samples = int(lengths.sum())
    rep = Report()
    emit = rep.emit
    eager = W.Basecaller(net, chunk=a.chunk, batch=a.batch)
    left, right = eager.left, eager.right
    plan = BC.chunk_plan(lengths, a.chunk, left, right, 3)
    n_chunks = int(plan.rows.shape[0])
    micro = -(-n_chunks // a.batch)
    emit("# chunked basecalling, RawCTCNet %d ch x (input block + %d blocks), %s, chunk=%d batch=%d, %s; reps=%d warmup=%d"
         % (C, len(layers), a.precision, a.chunk, a.batch, torch.cuda.get_device_name(0), a.reps, a.warmup))
    emit("receptive field (left, right) = (%d, %d); efficiency (chunk - left - right) / chunk = %.4f" % (left, right, eager.efficiency))
    emit("%d reads of %d..%d samples (int16 + scale / shift), %d samples kept, %d chunks = %d micro-batches (%d dead chunks)"
         % (a.reads, int(lengths.min()), int(lengths.max()), samples, n_chunks, micro, micro * a.batch - n_chunks))

    results = {}
    for name, graph in (("graph=False", False), ("graph=True", True)):
        bc = eager if not graph else W.Basecaller(net, chunk=a.chunk, batch=a.batch, graph=True)
        out = bc(raw, lengths, scale=scale, shift=shift)
        results[name] = out.logits
        lo, med, hi = wall_ms(lambda: bc(raw, lengths, scale=scale, shift=shift), a.reps, a.warmup)
        emit("%-12s call ms min / median / max = %.1f / %.1f / %.1f; %.1f ms per micro-batch; %.3e kept samples/s (median)"
             % (name, lo, med, hi, med / micro, samples / (med * 1e-3)))
    emit("graph=True logits bitwise equal to graph=False: %s" % bool(torch.equal(results["graph=False"], results["graph=True"])))
    del results

    # the pieces, on one full micro-batch of live chunks
    rows = plan.rows[:a.batch].to(dev)
    len_d = lengths.to(device=dev, dtype=torch.int32)
    frames_d = plan.frame_lengths.to(dev)
    x = torch.zeros(a.batch, 1, a.chunk, device=dev)
    x2 = x.view(a.batch, a.chunk)
    ms_gather = gpu_ms(lambda: BC.chunk_gather(raw, len_d, rows, a.chunk, x2, scale, shift, None), 50, 5)
    with torch.no_grad():
        y = net(x)
        ms_fwd = gpu_ms(lambda: net(x), 20, 3)
    logits = torch.zeros(a.reads, int(y.shape[1]), int(plan.frame_lengths.max()), device=dev)
    ms_stitch = gpu_ms(lambda: BC.chunk_stitch(y, rows, logits, frames_d, None), 50, 5)
    emit("per micro-batch, device events: gather %.4f ms, stitch %.4f ms, bare model(x) on [%d, 1, %d] %.3f ms (eager launches, "
         "frozen weights); (gather + stitch) / forward = %.4f" % (ms_gather, ms_stitch, a.batch, a.chunk, ms_fwd,
                                                                 (ms_gather + ms_stitch) / ms_fwd))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
