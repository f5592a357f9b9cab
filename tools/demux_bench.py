#!/usr/bin/env python3
"""Time barcode demultiplexing (csrc/wn_demux.hip: wn_demux_scores and wn_demux_pick) on the GPU at the shape of a multiplexed run:
4096 reads x 96 barcodes x both ends x a window of 150, porechop's costs.  Four pattern lengths, one per instantiation of the kernel: 24 (the
bare barcode; 32 rows), 40 (8-base flanks on both sides; 64 rows), 88 (32-base flanks; 96 rows) and 128 (52-base flanks; 128 rows).

What is timed.  wn_demux_scores through the C ABI on preallocated outputs (the kernel and its launch, nothing else), and demultiplex
through the Python surface (both launches, the output allocations, the fp32 copy of the scores); device events around `reps` calls
after `warmup` calls, reps raised until the window is at least --min-seconds.  A cell update is one (H, E, F) cell of one pattern
against one window column: reads x window x sum of the pattern lengths (both ends), computed here from the shapes.

The comparator.  The same three tables by a batched torch-op DP on the same GPU: the packed-word recurrence of DESIGN.md 7o run
anti-diagonal by anti-diagonal (the cells of one anti-diagonal are independent) over [reads, patterns, rows] int32 tensors, a dozen
elementwise torch kernels per anti-diagonal, in chunks of 1024 reads.  It is written for this tool only (patterns of one length, every
read at least a window long) and is not shipped; its tables must equal the kernel's exactly before any time is reported.
Usage: demux_bench.py [--reads N] [--barcodes N] [--window N] [--reps N] [--warmup N] [--min-seconds S] [--no-torch] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import wavenet_speech_amd as W  # noqa: E402
from wavenet_speech_amd import _lib  # noqa: E402
from wavenet_speech_amd._args import _p, _stream  # noqa: E402

from gputime import Report, timed  # noqa: E402

DEV = "cuda:0"
SHIFT, MASK, NEG = 10, 1023, -(3 << 29)


def gpu_ms(fn, reps, warmup, min_seconds):
    t = timed(fn, calls=reps, warmup=warmup, min_seconds=min_seconds)
    return t.median, t.calls


def torch_dp(window_rows, pat, costs, chunk=1024):
    """(score, start, end) [B, K] int32 in WINDOW coordinates of K patterns of one length P against B windows of one length, by
    anti-diagonals; window_rows [B, Wn] int32, pat [K, P] int32"""
    B, Wn = window_rows.shape
    K, P = pat.shape
    ma, mi, go, ge = (c << SHIFT for c in costs)
    rows = torch.arange(P + 1, device=DEV)
    pat_pad = torch.cat([torch.full((K, 1), -1, dtype=torch.int32, device=DEV), pat], 1)[None]       # row i holds label i - 1
    border = (-(go + (rows - 1) * ge) + MASK).to(torch.int32)                                         # H[i][0], i >= 1
    outs = []
    for c0 in range(0, B, chunk):
        win = window_rows[c0:c0 + chunk]
        shape = (win.shape[0], K, P + 1)
        neg = torch.full(shape, NEG, dtype=torch.int32, device=DEV)
        h1, h2, e1, f1 = neg.clone(), neg.clone(), neg.clone(), neg.clone()
        best = torch.full(shape[:2], -2 ** 31, dtype=torch.int32, device=DEV)
        best_j = torch.zeros(shape[:2], dtype=torch.int32, device=DEV)

        def shift(x):
            return torch.cat([neg[..., :1], x[..., :-1]], 2)

        for d in range(0, P + Wn + 1):
            j = d - rows                                                                              # the column of row i
            label = win[:, (j - 1).clamp(0, Wn - 1)]                                                  # [b, P + 1]
            sub = torch.where(label[:, None, :] == pat_pad, ma, mi).to(torch.int32)
            e = torch.maximum(torch.maximum(h1 - go, e1 - ge), neg)
            f = torch.maximum(torch.maximum(shift(h1) - go, shift(f1) - ge), neg)
            h = torch.maximum(torch.maximum(shift(h2) + sub, e), f)
            h[..., 0] = MASK - d if d <= Wn else NEG                                                  # row 0: (0, j)
            e[..., 0] = NEG
            f[..., 0] = NEG
            if 1 <= d <= P:                                                                           # column 0
                h[..., d] = border[d]
                f[..., d] = border[d]
                e[..., d] = NEG
            if 0 <= d - P <= Wn:
                cand = h[..., P]
                better = cand > best
                best = torch.where(better, cand, best)
                best_j = torch.where(better, torch.full_like(best_j, d - P), best_j)
            h2, h1, e1, f1 = h1, h, e, f
        outs.append((best >> SHIFT, MASK - (best & MASK), best_j))
    return tuple(torch.cat([o[i] for o in outs], 0) for i in range(3))


def torch_tables(labels, lengths, kit, window, costs):
    """the comparator's (score, start, end) [B, K] in read coordinates, both ends"""
    pat, _, _ = kit.on(torch.device(DEV))
    n = lengths.long()
    col = torch.arange(window, device=DEV)
    front = labels[:, :window]
    off = (n - window)[:, None]
    rear = labels.gather(1, off + col[None, :])
    s0, b0, e0 = torch_dp(front, pat[:kit.n_front], costs)
    s1, b1, e1 = torch_dp(rear, pat[kit.n_front:], costs)
    off = off.to(torch.int32)
    return torch.cat([s0, s1], 1), torch.cat([b0, b1 + off], 1), torch.cat([e0, e1 + off], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--barcodes", type=int, default=96)
    ap.add_argument("--window", type=int, default=150)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-op comparator")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "demux_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "demux_bench.py measures the GPU; there is no CPU path"
    lib = _lib.load()
    rng = np.random.default_rng(96)
    B, window = a.reads, a.window
    costs = (6, -12, 10, 4)
    n = rng.integers(max(400, window), 1201, B)
    host = np.zeros((B, 1200), dtype=np.int32)
    for b in range(B):
        host[b, :n[b]] = rng.integers(1, 5, n[b])
    labels, lengths = torch.from_numpy(host).to(DEV), torch.from_numpy(n.astype(np.int32)).to(DEV)
    codes = rng.integers(1, 5, (a.barcodes, 24))
    rep = Report()
    lines = ["# demultiplexing: %d reads of %d..1200 labels x %d barcodes x both ends x window %d, costs 3/-6/5/2, %s"
             % (B, max(400, window), a.barcodes, window, torch.cuda.get_device_name(0)),
             "%4s %5s %16s %6s %14s %18s %20s %16s %8s" % ("P", "form", "scores ms/call", "reps", "cell updates/s", "demultiplex ms/call",
                                                          "torch DP ms/call", "torch updates/s", "ratio")]
    for line in lines:
        rep.emit(line)
    for flank, form in ((0, "reg32"), (8, "reg64"), (32, "reg96"), (52, "reg128")):
        ff, rf = rng.integers(1, 5, flank).tolist(), rng.integers(1, 5, flank).tolist()
        kit = W.BarcodeSet([c.tolist() for c in codes], front_flank=ff, rear_flank=rf)
        P, K = kit.max_pattern_len, kit.n_patterns
        pat, plen, _ = kit.on(torch.device(DEV))
        out = [torch.empty(B, K, dtype=torch.int32, device=DEV) for _ in range(3)]
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)

        def scores():
            _lib.check(lib.wn_demux_scores(_p(labels), labels.stride(0), _p(lengths), _p(pat), pat.stride(0), _p(plen), B, labels.shape[1], K,
                                           kit.n_front, P, window, *costs, _p(out[0]), _p(out[1]), _p(out[2]), _p(bad), _stream()),
                       "wn_demux_scores")

        ms, reps = gpu_ms(scores, a.reps, a.warmup, a.min_seconds)
        ms_all, _ = gpu_ms(lambda: W.demultiplex(labels, lengths, kit, window=window), a.reps, a.warmup, a.min_seconds)
        cells = float(B) * window * float(kit.pattern_lengths.sum())
        assert int(bad[0]) == 0
        t_ms = t_rate = ratio = "not run"
        if not a.no_torch:
            want = torch_tables(labels, lengths, kit, window, costs)
            for got, ref, name in zip(out, want, ("score", "start", "end")):
                assert torch.equal(got, ref), "the comparator's %s differs from the kernel's" % name
            tm, _ = gpu_ms(lambda: torch_tables(labels, lengths, kit, window, costs), 1, 1, 0.0)
            t_ms, t_rate, ratio = "%.1f" % tm, "%.3g" % (cells / (tm * 1e-3)), "%.0fx" % (tm / ms)
        rep.emit("%4d %5s %16.3f %6d %14.3g %18.3f %20s %16s %8s" % (P, form, ms, reps, cells / (ms * 1e-3), ms_all, t_ms, t_rate, ratio))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
