#!/usr/bin/env python3
"""Time detect_events (csrc/wn_eventdetect.hip: scores and peaks, ranks, sums) on 256 reads x 2^18 samples and on 4 reads x 2^22
samples, float32 and int16, beside a device copy of the same signal bytes.  The reads are piecewise constant (dwell 4..16, levels
90 +- 12) plus Gaussian noise of sigma 1.5; max_events is L / 4, which holds every read whole.  Every figure is the median (and the
range) of `blocks` timed blocks of `runs` calls each, after one warm-up call per block; a call is the whole Python wrapper, its
six output and workspace allocations included.  Prints Gsamples/s of both.
Usage: events_detect_bench.py [runs [blocks]]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import wavenet_speech_amd as W  # noqa: E402

import gputime  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
BLOCKS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")


def reads(B, L, gen):
    dwell = torch.randint(4, 17, (B, L // 4), generator=gen, device=dev)
    level = 90.0 + 12.0 * torch.randn(B, L // 4, generator=gen, device=dev)
    rows = [torch.repeat_interleave(level[b], dwell[b])[:L] for b in range(B)]
    return torch.stack(rows) + 1.5 * torch.randn(B, L, generator=gen, device=dev)


def timed(fn):
    """(median, min, max) in ms per call over BLOCKS blocks of RUNS calls"""
    t = gputime.timed(fn, calls=RUNS, windows=BLOCKS, warm_each=1)
    return t.median, t.least, t.greatest


gen = torch.Generator(device=dev).manual_seed(0)
print("detect_events, defaults (windows 3 / 6): median (min .. max) of %d blocks of %d calls" % (BLOCKS, RUNS))
for B, L in ((256, 1 << 18), (4, 1 << 22)):
    x = reads(B, L, gen)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    raw = (x * 8.0).round().clamp(-32768, 32767).to(torch.int16)
    scale = torch.tensor([[0.125, 0.0]], device=dev).repeat(B, 1)
    for name, sig, ss in (("float32", x, None), ("int16", raw, scale)):
        ev = W.detect_events(sig, lengths, scale_shift=ss, max_events=L // 4)
        assert not bool(ev.truncated.any()) and int(ev.n_events.min()) > 0
        ms, lo, hi = timed(lambda: W.detect_events(sig, lengths, scale_shift=ss, max_events=L // 4))
        out = torch.empty_like(sig)
        copy_ms, copy_lo, copy_hi = timed(lambda: out.copy_(sig))
        n = B * L
        print("  %3d reads x 2^%d %-7s: %7.3f (%.3f .. %.3f) ms = %6.2f Gsamples/s   (%.1f events per read of mean length %.1f); "
              "device copy of the signal: %6.3f (%.3f .. %.3f) ms = %7.2f Gsamples/s, %.1f x"
              % (B, L.bit_length() - 1, name, ms, lo, hi, n / ms * 1e-6, float(ev.n_events.float().mean()), n / float(ev.n_events.sum()),
                 copy_ms, copy_lo, copy_hi, n / copy_ms * 1e-6, ms / copy_ms))
    W.check_device_flags()
