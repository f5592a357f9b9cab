#!/usr/bin/env python3
"""Time CTC forced alignment (csrc/wn_align.hip through wavenet_speech_amd.ctc_forced_align) on the GPU next to the loss-only
wn_ctc_loss call (dlogits = NULL: the forward recursion alone) on the SAME logits and labels: random [B, C, T] logits, C = 5,
B in {8, 32}, T in {1024, 4096}, L = T / 10 and L = 2047 (which 1024 frames cannot hold: those rows time the forward chains
alone).  Both run one workgroup per utterance and a chain of T sequential steps; the loss is the yardstick the alignment should not exceed.  Reports ms per batch (device events
around `reps` calls after `warmup` calls; buffers allocated outside the timed region for the loss, inside the Python call for
the alignment) and us per frame-step.  With --cpu-ref also the numpy float64 reference of the tests (tests/ctc_align_ref.py)
on ONE utterance per shape.  Usage: align_bench.py [--reps N] [--warmup N] [--cpu-ref] [--quick] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from wavenet_speech_amd import _lib  # noqa: E402
from wavenet_speech_amd import decoding as D  # noqa: E402
from wavenet_speech_amd.functional import _p, _stream  # noqa: E402

from gputime import Report, timed  # noqa: E402


def gpu_ms(fn, reps, warmup):
    return timed(fn, calls=reps, warmup=warmup).median


def loss_only(lib, x, labels, lens):
    """the loss-only wn_ctc_loss call (no gradient) with its buffers allocated once"""
    B, C, T = x.shape
    L = labels.shape[1]
    ws_bytes = lib.wn_ctc_workspace_bytes(B, C, T, L)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    nll = torch.empty(B, dtype=torch.float32, device=x.device)
    bad = torch.zeros(1, dtype=torch.int32, device=x.device)

    def call():
        _lib.check(lib.wn_ctc_loss(_p(x), _p(labels), _p(lens), None, B, C, T, L, 0, _p(nll), None, _p(ws), ws_bytes, _p(bad), _stream()),
                   "wn_ctc_loss")
    return call, nll, ws_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--quick", action="store_true", help="B=8, T=1024 only (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "align_bench.py measures the GPU; there is no CPU path"
    lib = _lib.load()
    C = 5
    Bs, Ts = ([8], [1024]) if a.quick else ([8, 32], [1024, 4096])
    rep = Report()
    lines = ["# CTC forced alignment next to the loss-only wn_ctc_loss call, C=%d, fp32 logits [B][C][T], %s; reps=%d warmup=%d"
             % (C, torch.cuda.get_device_name(0), a.reps, a.warmup),
             "%4s %5s %5s %13s %13s %12s %11s %10s %10s %15s" % ("B", "T", "L", "align ms/batch", "loss ms/batch", "align us/step",
                                                                 "align/loss", "align ws MB", "loss ws MB", "cpu-ref ms/utt")]
    for line in lines:
        rep.emit(line)
    for B in Bs:
        for T in Ts:
            for L in (max(T // 10, 1), 2047):
                g = torch.Generator().manual_seed(B * 100000 + T + L)
                xh = torch.randn(B, C, T, generator=g) * 1.5
                lh = torch.randint(1, C, (B, L), generator=g)
                x, labels = xh.to("cuda:0"), lh.to("cuda:0")
                lens = torch.full((B,), L, dtype=torch.int64, device="cuda:0")
                loss_call, nll, loss_ws = loss_only(lib, x, labels, lens)
                ms_loss = gpu_ms(loss_call, a.reps, a.warmup)
                ms_align = gpu_ms(lambda: D.ctc_forced_align(x, labels, lens), a.reps, a.warmup)
                out = D.ctc_forced_align(x, labels, lens)
                torch.cuda.synchronize()
                fits = bool(torch.isfinite(nll).all())              # L = 2047 does not fit in 1024 frames: the forward chains still run
                assert bool((out.score <= -nll * (1 - 1e-5)).all()) and bool(torch.isfinite(out.score).all()) == fits
                cpu = "" if fits else "(no alignment fits)"
                if a.cpu_ref:
                    from tests import ctc_align_ref as R
                    lp = R.log_softmax(xh[0].double().numpy())
                    t = time.perf_counter()
                    R.viterbi_align(lp, lh[0].tolist())
                    cpu = "%.0f %s" % ((time.perf_counter() - t) * 1e3, cpu)
                rep.emit("%4d %5d %5d %13.3f %13.3f %12.3f %11.2f %10.1f %10.1f %15s" % (
                    B, T, L, ms_align, ms_loss, ms_align * 1e3 / T, ms_align / ms_loss,
                    lib.wn_ctc_align_workspace_bytes(B, C, T, L) / 2**20, loss_ws / 2**20, cpu))
    torch.cuda.synchronize()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
