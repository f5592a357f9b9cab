#!/usr/bin/env python3
"""Time the event tables (csrc/wn_events.hip: wn_kmer_events, one memset and two launches) on the GPU next to the same k-mer
tables built from torch ops on the same device.  Shape: 32 reads of about 100 000 samples (about 16 700 bases each, dwell
uniform 6 +- 2, the "loader" window), generated on the device by ragged_reads; k = 5, frac_bits = 12, max_dwell = 255.

  wn_kmer_events          the C ABI call alone, buffers allocated beforehand: all per-event rows + read_counts + both tables
  kmer_events             what a user calls: the same plus its allocations, the zeroed tables and the flag's read-back
  torch ops               searchsorted (the event of every sample) + index_add_ per table column, int64, from the same float32
                          signal and starts; it makes kmer_stats with sum q^2 as ONE int64 column, the dwell histogram and no
                          per-event rows.  Its tables are compared with the kernel's before anything is timed.

Reports min / median / max ms per call (device events around every one of `reps` calls after `warmup` calls) and the signal
bytes the call reads per second at the median.  Writes its table to --out, by default profiles/rNN/events_bench.txt in the next
free rNN.
Usage: events_bench.py [--reps N] [--warmup N] [--reads B] [--bases N] [--out FILE]"""
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

K, FIRST, FRAC_BITS, MAX_DWELL = 5, 2, 12, 255


def gpu_ms(fn, reps, warmup):
    """(min, median, max) ms of one call"""
    return timed(fn, windows=reps, warmup=warmup)[:3]


def torch_tables(signal, signal_lengths, starts, kmers, live):
    """(stats [1024, 4] int64: events, samples, sum q, sum q^2; dwell_hist [1024, 256] int64) from torch ops"""
    B, L = signal.shape
    n_ev = kmers.shape[1]
    t = torch.arange(L, device=signal.device)[None, :].expand(B, L).contiguous()
    event = torch.searchsorted(starts[:, 1:].contiguous(), t.int(), right=True).clamp_(max=n_ev - 1)
    used = (t < signal_lengths[:, None]) & live.gather(1, event)
    code = kmers.gather(1, event)[used]
    q = torch.round(signal.double() * float(1 << FRAC_BITS)).long()[used]
    stats = torch.zeros(4 ** K, 4, dtype=torch.int64, device=signal.device)
    ones = torch.ones_like(code)
    stats[:, 1].index_add_(0, code, ones)
    stats[:, 2].index_add_(0, code, q)
    stats[:, 3].index_add_(0, code, q * q)
    ev_code = kmers[live]
    stats[:, 0].index_add_(0, ev_code, torch.ones_like(ev_code))
    length = (starts[:, 1:] - starts[:, :-1])[live].long().clamp_(max=MAX_DWELL)
    hist = torch.zeros(4 ** K * (MAX_DWELL + 1), dtype=torch.int64, device=signal.device)
    hist.index_add_(0, ev_code * (MAX_DWELL + 1) + length, torch.ones_like(length))
    return stats, hist.view(4 ** K, MAX_DWELL + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reads", type=int, default=32)
    ap.add_argument("--bases", type=int, default=16700, help="about 6 samples each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "events_bench.py measures the GPU; there is no CPU path"
    assert a.reps >= 20, "the median of at least 20 runs"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    reads = S.ragged_reads(a.reads, (a.bases, a.bases + 200), ("uniform", 6, 2), "loader", generator=g, device=dev)
    signal = reads.signal[:, 0]
    B, L = signal.shape
    n_ev = reads.dwell.shape[1]
    live = torch.arange(n_ev, device=dev)[None, :] < (reads.base_lengths.long() - 8)[:, None]
    kmers = S.ragged_kmers(reads.bases, reads.base_lengths, 2)

    def user():
        return W.kmer_events(reads.signal, reads.signal_lengths, reads.bases, reads.base_lengths, starts=reads.starts, k=K, first=FIRST,
                             frac_bits=FRAC_BITS, max_dwell=MAX_DWELL)

    ev = user()
    stats, hist = torch_tables(signal, reads.signal_lengths, reads.starts, kmers, live)
    W.check_device_flags()
    assert torch.equal(ev.kmer_stats[:, :3], stats[:, :3]) and torch.equal(ev.kmer_stats[:, 3] + (ev.kmer_stats[:, 4] << 32), stats[:, 3])
    assert torch.equal(ev.dwell_hist, hist)
    samples, events = int(ev.read_counts[:, 3].sum()), int(ev.read_counts[:, 0].sum())

    lib = _lib.load()
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    rows = [torch.empty(B, n_ev, **i32) for _ in range(3)] + [torch.empty(B, n_ev, **i64) for _ in range(2)]
    counts, bad = torch.empty(B, 4, **i32), torch.zeros(1, **i32)
    t_stats, t_hist = torch.zeros(4 ** K, 5, **i64), torch.zeros(4 ** K, MAX_DWELL + 1, **i64)
    ws_bytes = lib.wn_kmer_events_workspace_bytes(B, n_ev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    n_events = torch.full((B,), n_ev, **i32)
    bases, starts = reads.bases.contiguous(), reads.starts.contiguous()

    def abi(rows=rows):
        _lib.check(lib.wn_kmer_events(_p(signal), 0, signal.stride(0), _p(reads.signal_lengths), None, _p(starts),
                                      _p(starts.data_ptr() + 4), starts.stride(0), 1, 1, 0, _p(bases), bases.stride(0),
                                      _p(reads.base_lengths), _p(n_events), B, L, int(bases.shape[1]), n_ev, K, FIRST, FRAC_BITS, MAX_DWELL,
                                      _p(rows[0]), _p(rows[1]), _p(rows[2]), _p(rows[3]), _p(rows[4]), _p(counts), _p(t_stats),
                                      _p(t_hist), _p(ws), ws_bytes, _p(bad), _stream()), "wn_kmer_events")

    abi()
    torch.cuda.synchronize()
    assert torch.equal(t_stats, ev.kmer_stats) and torch.equal(rows[3], ev.sum) and int(bad) == 0
    work = [("wn_kmer_events (C ABI)", abi), ("wn_kmer_events, tables only", lambda: abi([None] * 5)), ("kmer_events (Python)", user),
            ("torch ops", lambda: torch_tables(signal, reads.signal_lengths, reads.starts, kmers, live))]
    rep = Report()
    lines = ["# event tables: %d reads, %d samples (%.1f MB of float32 signal), %d events, k=%d, frac_bits=%d, max_dwell=%d, %s; "
             "reps=%d warmup=%d; ms per call: min / median / max" % (B, samples, samples * 4 / 1e6, events, K, FRAC_BITS, MAX_DWELL,
                                                                    torch.cuda.get_device_name(0), a.reps, a.warmup),
             "%-30s %28s %14s %10s" % ("form", "ms", "signal GB/s", "vs torch")]
    for line in lines:
        rep.emit(line)
    results = [(name, gpu_ms(fn, a.reps, a.warmup)) for name, fn in work]
    base = results[-1][1][1]
    for name, t in results:
        line = "%-30s %28s %14.1f %10.2f" % (name, "%.3f / %.3f / %.3f" % t, samples * 4 / (t[1] * 1e-3) / 1e9, base / t[1])
        rep.emit(line)
    W.check_device_flags()
    out = a.out or os.path.join(next_profile_dir(), "events_bench.txt")
    rep.save(out)
    print("wrote", out)


if __name__ == "__main__":
    main()
