#!/usr/bin/env python3
"""Time the signal-to-base alignment (csrc/wn_sigalign.hip: wn_signal_align, one launch, one workgroup per read) on the GPU, and
run three rounds of Viterbi training with it.

Timing.  Reads generated on the device by ragged_reads (gamma dwell of about 8 samples per k-mer, the "loader" window), B in
{32, 256} reads of about 2 000 and about 16 000 k-mers, band in {128, 512}; device events around the C ABI call alone (buffers
allocated beforehand), min / median / max ms over `reps` calls after `warmup` calls (a tenth of both for the long reads), with the
samples per second at the median, the reads whose band_hits are not 0 and the share of samples put in their true k-mer.

Training.  32 reads of about 2 000 k-mers; the table starts with every mean moved by one stdv of its k-mer (random sign and size,
N(0, 1) stdvs); three rounds of signal_align -> kmer_events -> fit_kmer_model -> signal_model, each printing the total cost in nats
and the worst and mean |mean - true mean| over the k-mers with at least 100 samples.

Writes its table to --out, by default profiles/rNN/signal_align_bench.txt in the next free rNN.
Usage: signal_align_bench.py [--reps N] [--warmup N] [--out FILE] [--quick]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import wavenet_speech_amd as W  # noqa: E402
from wavenet_speech_amd import _lib  # noqa: E402
from wavenet_speech_amd import synthetic as S  # noqa: E402
from wavenet_speech_amd.functional import _p, _stream  # noqa: E402

from gputime import Report, next_profile_dir, timed  # noqa: E402

FIRST = 2
DWELL = ("gamma", 4.0, 2000.0, 4000.0)          # mean 8 samples, shape 4


def gpu_ms(fn, reps, warmup):
    """(min, median, max) ms of one call"""
    return timed(fn, windows=reps, warmup=warmup)[:3]


def time_shape(lib, model, B, bases, band, reps, warmup, dev):
    g = torch.Generator().manual_seed(1)
    reads = S.ragged_reads(B, (bases, bases + bases // 50 + 2), DWELL, "loader", generator=g, device=dev)
    signal, labels = reads.signal[:, 0], reads.bases.contiguous()
    L, N = int(signal.shape[1]), int(labels.shape[1]) - 4 - 2 * FIRST
    i32 = dict(dtype=torch.int32, device=dev)
    starts, score = torch.empty(B, N + 1, **i32), torch.empty(B, dtype=torch.int64, device=dev)
    hits, states, bad = torch.empty(B, **i32), torch.empty(B, L, **i32), torch.zeros(1, **i32)
    ws_bytes = lib.wn_signal_align_workspace_bytes(B, L, band)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    table = model.on(dev)

    def abi():
        _lib.check(lib.wn_signal_align(_p(signal), 0, signal.stride(0), _p(reads.signal_lengths), None, _p(labels), labels.stride(0),
                                       _p(reads.base_lengths), _p(table), B, L, int(labels.shape[1]), N, model.k, FIRST, model.frac_bits,
                                       model.weight_shift, 2 ** 31 - 1, band, _p(starts), _p(score), _p(hits), _p(states), _p(ws),
                                       ws_bytes, _p(bad), _stream()), "wn_signal_align")

    t = gpu_ms(abi, reps, warmup)
    assert int(bad) == 0
    samples, kmers = int(reads.signal_lengths.sum()), int((reads.base_lengths.long() - 8).sum())
    inside = reads.sample_kmer >= 0
    agree = float((states == reads.sample_kmer)[inside].double().mean())
    return "%5d %8d %6d %10d %10d %8.1f %30s %10.2f %8d %10.4f" % (B, bases, band, samples, kmers, ws_bytes / 2 ** 20, "%.3f / %.3f / %.3f" % t,
                                                                 samples / (t[1] * 1e-3) / 1e6, int((hits != 0).sum()), agree)


def training(dev, rounds=3):
    truth = S.standin_kmer_table()
    tm, ts = truth[0].double(), truth[1].double()
    g = torch.Generator().manual_seed(2)
    reads = S.ragged_reads(32, (2000, 2040), DWELL, "loader", truth, generator=g, device=dev)
    means = tm + ts * torch.randn(tm.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    stdvs = ts.clone()
    lines = ["# Viterbi training: 32 reads, %d samples, %d k-mers; means start one stdv off (worst %.3f, mean %.3f); band 512"
             % (int(reads.signal_lengths.sum()), int((reads.base_lengths.long() - 8).sum()), float((means - tm).abs().max()),
                float((means - tm).abs().mean())),
             "%6s %16s %10s %12s %12s %12s %10s" % ("round", "cost, nats", "k-mers", "worst |dm|", "mean |dm|", "in true kmer", "band hits")]
    inside = reads.sample_kmer >= 0
    for r in range(rounds + 1):                                      # the last pass only scores the last table
        model = W.signal_model(means, stdvs)
        al = W.signal_align(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, model, first=FIRST, band=512, want_states=True)
        ev = W.kmer_events(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, starts=al.starts, k=al.k, first=al.first)
        W.check_device_flags()
        fm, fs, counts = W.fit_kmer_model(ev.kmer_stats, min_count=100, prior=(means, stdvs))
        used = counts >= 100
        agree = float((al.states == reads.sample_kmer)[inside].double().mean())
        lines.append("%6d %16.1f %10d %12.4f %12.4f %12.4f %10d" % (r, float(al.nats.sum()), int(used.sum()), float((means - tm).abs()[used].max()),
                                                                   float((means - tm).abs()[used].mean()), agree, int(al.band_hits.sum())))
        means, stdvs = fm, fs.clamp(min=0.05)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the short reads only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "signal_align_bench.py measures the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    model = W.signal_model(*S.standin_kmer_table())
    rep = Report()
    lines = ["# signal_align: k=%d, frac_bits=%d, weight_shift=%d, dwell %s, %s; device events around wn_signal_align; reps=%d warmup=%d "
             "(long reads: %d and %d); ms per call: min / median / max" % (model.k, model.frac_bits, model.weight_shift, DWELL,
                                                                          torch.cuda.get_device_name(0), a.reps, a.warmup,
                                                                          max(a.reps // 10, 2), max(a.warmup // 3, 1)),
             "%5s %8s %6s %10s %10s %8s %30s %10s %8s %10s" % ("reads", "bases", "band", "samples", "k-mers", "ws MiB", "ms", "Msample/s",
                                                             "hit", "true kmer")]
    for line in lines:
        rep.emit(line)
    for bases in (2000,) if a.quick else (2000, 16000):
        for B in (32, 256):
            for band in (128, 512):
                long_read = bases > 4000
                line = time_shape(lib, model, B, bases, band, max(a.reps // 10, 2) if long_read else a.reps,
                                  max(a.warmup // 3, 1) if long_read else a.warmup, dev)
                rep.emit(line)
    for line in training(dev):
        rep.emit(line)
    W.check_device_flags()
    out = a.out or os.path.join(next_profile_dir(), "signal_align_bench.txt")
    rep.save(out)
    print("wrote", out)


if __name__ == "__main__":
    main()
