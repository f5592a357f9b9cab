#!/usr/bin/env python3
"""Time the event alignment (csrc/wn_eventalign.hip: wn_event_align, one launch, one workgroup per read) on the GPU against the
signal alignment it extends, measure how well both place the samples, and re-estimate the move probabilities twice.

Reads.  ragged_reads draws bases and dwells on the device (gamma dwell of about 8 samples per k-mer, the "loader" window); the
signal is formed here from its sample_kmer: the stand-in table's mean of the sample's k-mer (the NOISE-FREE form) plus Gaussian
noise of sigma 1.5 or 3.0.  B in {32, 256} reads of about 2 000 and about 16 000 k-mers, band in {128, 512}: the shapes of
tools/signal_align_bench.py.

Timing.  detect_events on the noisy reads (defaults) gives the event tables; wn_event_align is timed on them through the C ABI with
every buffer allocated beforehand and device events around the call, beside wn_signal_align on the same reads' raw samples in
their noise-free form (the noisy reads' events are fewer than their k-mers, so signal_align on the events has no alignment at all).
Both are reported as median (min .. max) ms per call over `blocks` blocks of `calls` calls, each block after one warm-up call and
timed as a whole (a tenth of the calls, at least one, for signal_align on the long reads).

Agreement.  The share of samples that the alignment's starts put into the k-mer the generator drew them from, at sigma 1.5 and
3.0, beside signal_align's on the noise-free samples.

Moves.  32 reads of about 2 000 k-mers at sigma 1.5, band 512: align with DEFAULT_MOVES, fit_moves, align, fit_moves, align.

Writes its table to --out, by default profiles/rNN/event_align_bench.txt in the next free rNN.
Usage: event_align_bench.py [--blocks N] [--calls N] [--out FILE] [--quick]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import wavenet_speech_amd as W  # noqa: E402
from wavenet_speech_amd import _lib  # noqa: E402
from wavenet_speech_amd import synthetic as S  # noqa: E402
from wavenet_speech_amd._args import _p, _stream  # noqa: E402

from gputime import Report, next_profile_dir, timed  # noqa: E402

FIRST, K = 2, 5
DWELL = ("gamma", 4.0, 2000.0, 4000.0)          # mean 8 samples, shape 4


def block_ms(fn, blocks, calls):
    """median, min, max over `blocks` of the ms per call of a block of `calls` calls, each block after one warm-up call"""
    t = timed(fn, calls=calls, windows=blocks, warm_each=1)
    return t.median, t.least, t.greatest


def make_reads(B, bases, seed, dev):
    """(reads, clean [B, L] float32, N): the noise-free signal of ragged_reads' own k-mers"""
    g = torch.Generator().manual_seed(seed)
    reads = S.ragged_reads(B, (bases, bases + bases // 50 + 2), DWELL, "loader", generator=g, device=dev)
    labels = reads.bases.long()
    N = int(labels.shape[1]) - (K - 1) - 2 * FIRST
    code = torch.zeros(B, N, dtype=torch.long, device=dev)
    for i in range(K):
        code = code * 4 + (labels[:, FIRST + i:FIRST + i + N] - 1).clamp(0, 3)
    means = S.standin_kmer_table()[0].to(dev).float()
    state = reads.sample_kmer.long().clamp(min=0)
    clean = means[torch.gather(code, 1, state.clamp(max=N - 1))]
    clean = torch.where(reads.sample_kmer >= 0, clean, torch.zeros_like(clean)).contiguous()
    return reads, clean, N


def noisy(clean, sigma, seed):
    g = torch.Generator(device=clean.device).manual_seed(seed)
    return (clean + sigma * torch.randn(clean.shape, generator=g, device=clean.device)).contiguous()


def share_in_true_kmer(starts, reads, N):
    """the share of samples inside a read's k-mers that `starts` puts into the generator's own k-mer"""
    L = reads.sample_kmer.shape[1]
    t = torch.arange(L, device=starts.device)[None, :].expand(starts.shape[0], L).contiguous()
    state = torch.searchsorted(starts[:, :N + 1].contiguous(), t.int(), right=True) - 1
    inside = reads.sample_kmer >= 0
    return float((state == reads.sample_kmer)[inside].double().mean())


def model_of(sigma):
    means, _ = S.standin_kmer_table()
    return W.signal_model(means, torch.full_like(means, sigma))


def time_shape(lib, B, bases, band, blocks, calls, dev):
    reads, clean, N = make_reads(B, bases, 1, dev)
    labels, ll, L = reads.bases.contiguous(), reads.base_lengths, int(clean.shape[1])
    model = model_of(1.5)
    table = model.on(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    cols = {}
    for sigma in (1.5, 3.0):
        ev = W.detect_events(noisy(clean, sigma, 7), reads.signal_lengths, max_events=L // 4)
        assert not bool(ev.truncated.any())
        al = W.event_align(ev, labels, ll, model_of(sigma), first=FIRST, band=band)
        cols[sigma] = (share_in_true_kmer(al.starts, reads, N), int((al.band_hits != 0).sum()), int((al.score == 2 ** 63 - 1).sum()),
                       int(ev.held.sum()), int(ev.held.max()), ev)
    ev = cols[1.5][5]
    M, held = ev.max_events, ev.held.contiguous()
    costs = W.move_costs(W.DEFAULT_MOVES, model.cost_bits)
    starts, score = torch.empty(B, N + 1, **i32), torch.empty(B, dtype=torch.int64, device=dev)
    hits, counts, bad = torch.empty(B, **i32), torch.empty(B, 4, **i32), torch.zeros(1, **i32)
    ws_bytes = lib.wn_event_align_workspace_bytes(B, M, band)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def event_abi():
        _lib.check(lib.wn_event_align(_p(held), _p(ev.starts), _p(ev.sum), _p(ev.sumsq), _p(labels), labels.stride(0), _p(ll), _p(table), B, M,
                                      int(labels.shape[1]), N, K, FIRST, model.frac_bits, model.weight_shift, 2 ** 31 - 1, band, costs[0],
                                      costs[1], costs[2], costs[3], _p(starts), _p(score), None, _p(counts), _p(hits), _p(ws), ws_bytes, _p(bad),
                                      _stream()), "wn_event_align")

    te = block_ms(event_abi, blocks, calls)
    assert int(bad) == 0
    s_starts, s_hits = torch.empty(B, N + 1, **i32), torch.empty(B, **i32)
    s_bytes = lib.wn_signal_align_workspace_bytes(B, L, band)
    s_ws = torch.empty(s_bytes, dtype=torch.uint8, device=dev)

    def signal_abi():
        _lib.check(lib.wn_signal_align(_p(clean), 0, clean.stride(0), _p(reads.signal_lengths), None, _p(labels), labels.stride(0), _p(ll),
                                       _p(table), B, L, int(labels.shape[1]), N, K, FIRST, model.frac_bits, model.weight_shift, 2 ** 31 - 1,
                                       band, _p(s_starts), _p(score), _p(s_hits), None, _p(s_ws), s_bytes, _p(bad), _stream()), "wn_signal_align")

    long_read = bases > 4000
    ts = block_ms(signal_abi, max(blocks // 2, 3) if long_read else blocks, max(calls // 10, 1) if long_read else calls)
    assert int(bad) == 0
    s_share = share_in_true_kmer(s_starts, reads, N)
    fmt = "%.3f (%.3f .. %.3f)"
    a, c = cols[1.5], cols[3.0]
    return "%5d %7d %5d %10d %9d %8d %26s %8.3f %26s %8.3f %7.4f %4d %4d %7.4f %4d %4d %7.4f" % (
        B, bases, band, int(reads.signal_lengths.sum()), a[3], a[4], fmt % te, te[0] * 1e3 / a[4], fmt % ts,
        ts[0] * 1e3 / int(reads.signal_lengths.max()), a[0], a[1], a[2], c[0], c[1], c[2], s_share)


def move_rounds(dev, rounds=2):
    reads, clean, N = make_reads(32, 2000, 2, dev)
    model = model_of(1.5)
    ev = W.detect_events(noisy(clean, 1.5, 9), reads.signal_lengths, max_events=int(clean.shape[1]) // 4)
    lines = ["# fit_moves: 32 reads, %d samples, %d events, %d k-mers, sigma 1.5, band 512" % (int(reads.signal_lengths.sum()), int(ev.held.sum()),
                                                                                              int((reads.base_lengths.long() - 8).sum())),
             "%6s %44s %16s %12s %10s" % ("round", "moves aligned with (stay, step, skip, skip 2)", "cost, nats", "in true kmer", "band hits")]
    moves = W.DEFAULT_MOVES
    for r in range(rounds + 1):
        al = W.event_align(ev, reads.bases, reads.base_lengths, model, first=FIRST, band=512, moves=moves)
        W.check_device_flags()
        lines.append("%6d %44s %16.1f %12.4f %10d" % (r, "%.4f %.4f %.4f %.4f" % tuple(moves), float(al.nats.sum()),
                                                      share_in_true_kmer(al.starts, reads, N), int(al.band_hits.sum())))
        moves = W.fit_moves(al.moves)
    lines.append("# the moves fitted last: %.4f %.4f %.4f %.4f" % tuple(moves))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the short reads only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "event_align_bench.py measures the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rep = Report()
    lines = ["# event_align against signal_align: k=%d, dwell %s, %s; device events around the C call, buffers allocated beforehand; "
             "median (min .. max) ms per call over %d blocks of %d calls (signal_align on the long reads: fewer, see the tool)"
             % (K, DWELL, torch.cuda.get_device_name(0), a.blocks, a.calls),
             "# events: detect_events' defaults on the reads at sigma 1.5; us/step: the median over the longest read's events (samples); "
             "true: share of samples in the generator's own k-mer; hit: reads with band hits; none: reads without an alignment",
             "%5s %7s %5s %10s %9s %8s %26s %8s %26s %8s %7s %4s %4s %7s %4s %4s %7s" % (
                 "reads", "bases", "band", "samples", "events", "longest", "event_align ms", "us/step", "signal_align (clean) ms", "us/step",
                 "true1.5", "hit", "none", "true3.0", "hit", "none", "sa true")]
    for line in lines:
        rep.emit(line)
    for bases in (2000,) if a.quick else (2000, 16000):
        for B in (32, 256):
            for band in (128, 512):
                line = time_shape(lib, B, bases, band, a.blocks, a.calls, dev)
                rep.emit(line)
    for line in move_rounds(dev):
        rep.emit(line)
    W.check_device_flags()
    out = a.out or os.path.join(next_profile_dir(), "event_align_bench.txt")
    rep.save(out)
    print("wrote", out)


if __name__ == "__main__":
    main()
