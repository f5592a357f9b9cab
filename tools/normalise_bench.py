#!/usr/bin/env python3
"""Time read normalisation (wavenet_speech_amd.normalise.read_med_mad, csrc/wn_select.hip) on the GPU with device events: min /
median / max of `reps` calls after `warmup`, on
  * the 48 int16 reads of tools/basecall_bench.py (20000..120000 samples), once with concentrated values as the read generator
    produces them (uniform in 300..700 there) and once with uniform random int16 over the whole range (the contention case);
  * 8 fp32 reads of 4 M samples;
  * with --large-int16, 8 int16 reads of 4 M samples, concentrated and uniform: beyond the launch-bound sizes above, where
    same-bin contention in the LDS histograms would show.
Next to each: the stock-torch baseline on the same device (padded torch.sort with a sentinel past each length, then indexing at
the two middle ranks, for the median and again for the deviations), and the simple model "passes x bytes read / time" in GB/s
(every pass of a selection streams the live samples once: 2 + 4 passes for int16, 4 + 4 for fp32).  The results of the two are
compared for exact equality.
Usage: normalise_bench.py [--reps N] [--warmup N] [--large-int16] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from wavenet_speech_amd import normalise as N  # noqa: E402

from gputime import Report, timed  # noqa: E402


def event_ms(fn, reps, warmup):
    """device time of every one of `reps` calls"""
    return timed(fn, windows=reps, warmup=warmup)[:3]


def sort_med_mad(signal, lengths):
    """stock torch: sort the padded batch with a sentinel above every value past each length, index the two middle ranks"""
    x = signal.float()
    past = torch.arange(x.shape[1], device=x.device)[None, :] >= lengths[:, None]
    n = lengths.to(torch.int64)
    lo, hi = ((n - 1) // 2)[:, None], (n // 2)[:, None]

    def middle(v):
        s = torch.sort(v.masked_fill(past, float("inf")), dim=1)[0]
        return ((s.gather(1, lo) + s.gather(1, hi)) * 0.5)[:, 0]

    med = middle(x)
    return med, middle((x - med[:, None]).abs())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--large-int16", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "normalise_bench.py measures the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rep = Report()
    emit = rep.emit
    g = torch.Generator().manual_seed(1)                              # the reads of tools/basecall_bench.py
    lengths48 = torch.randint(20000, 120001, (48,), generator=g)
    concentrated = torch.randint(300, 700, (48, int(lengths48.max())), generator=g).to(torch.int16)
    uniform = torch.randint(-32768, 32768, concentrated.shape, generator=g).to(torch.int16)
    lengths8 = torch.full((8,), 4 * 1024 * 1024, dtype=torch.int64)
    big = torch.randn(8, int(lengths8.max()), generator=g) * 12.0 + 90.0
    emit("# read_med_mad on %s, device events, reps=%d warmup=%d; TILE=%d" % (torch.cuda.get_device_name(0), a.reps, a.warmup, N.TILE))
    work = [("48 int16 reads, concentrated (300..700)", concentrated, lengths48, 2 + 4),
            ("48 int16 reads, uniform over int16", uniform, lengths48, 2 + 4),
            ("8 fp32 reads of 4 M samples", big, lengths8, 4 + 4)]
    if a.large_int16:
        work.append(("8 int16 reads of 4 M samples, concentrated (300..700)", torch.randint(300, 700, big.shape, generator=g).to(torch.int16),
                     lengths8, 2 + 4))
        work.append(("8 int16 reads of 4 M samples, uniform over int16", torch.randint(-32768, 32768, big.shape, generator=g).to(torch.int16),
                     lengths8, 2 + 4))
    for name, sig, lengths, passes in work:
        sig, len_d = sig.to(dev), lengths.to(device=dev, dtype=torch.int32)
        B = int(sig.shape[0])
        bad = torch.zeros(1, dtype=torch.int32, device=dev)          # the caller's counter: no host check inside the timed call
        ws = (N.select_workspace(B, 2, sig.dtype, False, dev), N.select_workspace(B, 2, sig.dtype, True, dev))
        med, mad = N.read_med_mad(sig, len_d, bad=bad, workspaces=ws)
        want_med, want_mad = sort_med_mad(sig, len_d)
        same = bool(torch.equal(med, want_med) and torch.equal(mad, want_mad)) and int(bad.item()) == 0
        ours = event_ms(lambda: N.read_med_mad(sig, len_d, bad=bad, workspaces=ws), a.reps, a.warmup)
        base = event_ms(lambda: sort_med_mad(sig, len_d), a.reps, a.warmup)
        live_bytes = int(lengths.sum()) * sig.element_size()
        emit("%s: %d..%d samples, %.1f MB live" % (name, int(lengths.min()), int(lengths.max()), live_bytes / 1e6))
        emit("  read_med_mad     ms min / median / max = %.3f / %.3f / %.3f; model %d passes x %.1f MB / median = %.0f GB/s"
             % (ours + (passes, live_bytes / 1e6, passes * live_bytes / (ours[1] * 1e-3) / 1e9)))
        emit("  torch.sort based ms min / median / max = %.3f / %.3f / %.3f; %.1f x read_med_mad (median); results equal: %s"
             % (base + (base[1] / ours[1], same)))
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
