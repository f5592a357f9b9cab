#!/usr/bin/env python3
"""Time read mapping (csrc/wn_readmap.hip: wn_minimizers, wn_read_seeds with its sort of the anchor rows, wn_chain) on the GPU at the
shape of a bacterial run: 4096 reads of 400..1200 labels with 8 % errors (deletions, insertions, substitutions in equal parts, both
strands) against a random reference of 4.6 M bases, at the defaults (k 15, w 10, max_occ 8, h 64, 4096 anchors per read).

What is timed.  Each stage through the C ABI on preallocated outputs (the kernel and its launch, nothing else), and map_reads
through the Python surface (all three with the allocations); device events
around `reps` calls after `warmup` calls, reps raised until the window is at least --min-seconds; every window is taken --repeats
times and the median is reported with the least and the greatest.  The index of the reference is built once and timed with a
host clock around a synchronise.  Anchors are the kept anchors of all reads; an evaluated predecessor pair is one (i, j) the chain
recurrence looks at: per strand of m anchors sum_i min(i, h), computed here from the anchor rows.

The comparator.  The same chain table (f and pred of every anchor) by a batched torch-op DP on the same GPU: one step per anchor
index over all reads at once, the h predecessors gathered as [reads, h] tensors, the lexicographic maximum as one packed int64
word, some twenty elementwise torch kernels per step.  It is written for this tool only and is not shipped; its table must equal
the kernel's exactly before any time is printed.
Usage: readmap_bench.py [--reads N] [--reference N] [--reps N] [--warmup N] [--min-seconds S] [--repeats N] [--no-torch] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gputime import Report, timed  # noqa: E402

DEFAULTS = dict(h=64, max_dist=5000, bandwidth=500, gap_base=2, gap_log=8)


def make_reads(rng, ref, count, lo=400, hi=1200, rate=0.08):
    """reads drawn from `ref` (numpy int32) on alternating strands with errors at `rate`, a third each: (labels [count, width], lengths)"""
    out = []
    for b in range(count):
        n = int(rng.integers(lo, hi + 1))
        start = int(rng.integers(0, len(ref) - n + 1))
        seq = ref[start:start + n]
        u = rng.random(n)
        sub = (u >= 2 * rate / 3) & (u < rate)
        seq = np.where(sub, (seq - 1 + rng.integers(1, 4, n)) % 4 + 1, seq)
        copies = np.where(u < rate / 3, 0, np.where(u < 2 * rate / 3, 2, 1))     # deleted, followed by an inserted base, kept
        source = np.repeat(np.arange(n), copies)
        seq = seq[source]
        inserted = np.concatenate([[False], source[1:] == source[:-1]])[:len(seq)]
        seq = np.where(inserted, rng.integers(1, 5, len(seq)), seq)
        out.append((5 - seq[::-1]) if b & 1 else seq)
    width = max(len(s) for s in out)
    labels = np.zeros((count, width), dtype=np.int32)
    for b, s in enumerate(out):
        labels[b, :len(s)] = s
    return labels, np.array([len(s) for s in out], dtype=np.int32)


def torch_chain(keys, n_anchors, k, h=64, max_dist=5000, bandwidth=500, gap_base=2, gap_log=8):
    """(f, pred) [B, cap] int32 of sorted anchor rows by torch ops, INT_MIN / -1 past n_anchors: the comparator"""
    dev = keys.device
    B, cap = keys.shape
    steps = int(n_anchors.max()) if B else 0
    strand, r, q = (keys >> 43) & 1, (keys >> 16) & ((1 << 27) - 1), keys & 0xFFFF
    f = torch.full((B, cap), -2 ** 31, dtype=torch.int64, device=dev)
    pred = torch.full((B, cap), -1, dtype=torch.int64, device=dev)
    d = torch.arange(h, device=dev)[None, :]
    live_all = torch.arange(cap, device=dev)[None, :] < n_anchors[:, None].long()
    for i in range(steps):
        j = (i - 1 - d).expand(B, h)
        jc = j.clamp(min=0)
        dr, dq = r[:, i:i + 1] - r.gather(1, jc), q[:, i:i + 1] - q.gather(1, jc)
        dd = (dr - dq).abs()
        ok = (j >= 0) & (strand.gather(1, jc) == strand[:, i:i + 1]) & (dr > 0) & (dr <= max_dist) & (dq > 0) & (dq <= max_dist) & (dd <= bandwidth)
        log2 = torch.floor(torch.log2(dd.clamp(min=1).double())).long()              # exact: dd < 2^27 is a double's integer
        gap = torch.where(dd > 0, gap_base * dd + gap_log * log2, torch.zeros_like(dd))
        cand = f.gather(1, jc) + 16 * torch.minimum(torch.minimum(dr, dq), torch.full_like(dr, k)) - gap
        word = torch.where(ok, cand * 2048 + (2047 - d), torch.full_like(cand, -2 ** 62))
        best = word.max(1).values
        score, dist = best >> 11, 2047 - (best & 2047)
        ext = score > 16 * k                                                          # a fresh start beats an equal extension
        live = live_all[:, i]
        f[:, i] = torch.where(live, torch.where(ext, score, torch.full_like(score, 16 * k)), f[:, i])
        pred[:, i] = torch.where(live & ext, i - 1 - dist, pred[:, i])
    return f.int(), pred.int()


def pairs_evaluated(keys, n_anchors, h):
    """sum over reads and strands of sum_i min(i, h)"""
    live = torch.arange(keys.shape[1], device=keys.device)[None, :] < n_anchors[:, None].long()
    rev = (((keys >> 43) & 1) == 1) & live
    total = 0
    for m in ((live & ~rev).sum(1), rev.sum(1)):
        m = m.long()
        total += int(torch.where(m <= h, m * (m - 1) // 2, h * (h - 1) // 2 + (m - h) * h).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--reference", type=int, default=4600000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-op comparator")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "readmap_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "readmap_bench.py measures the GPU; there is no CPU path"
    import wavenet_speech_amd as W
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(46)
    ref = rng.integers(1, 5, a.reference).astype(np.int32)
    host_labels, host_lengths = make_reads(rng, ref, a.reads)
    labels, lengths = torch.from_numpy(host_labels).to(dev), torch.from_numpy(host_lengths).to(dev)
    B, L = labels.shape
    k, w, max_occ, cap = 15, 10, 8, 4096
    ref_dev = torch.from_numpy(ref).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = W.read_index(ref_dev)
    torch.cuda.synchronize()
    index_ms = 1e3 * (time.perf_counter() - t0)                                       # the first call: code objects load here too
    t0 = time.perf_counter()
    index = W.read_index(ref_dev)
    torch.cuda.synchronize()
    index_ms2 = 1e3 * (time.perf_counter() - t0)

    code, flag = torch.empty(B, L, dtype=torch.int32, device=dev), torch.empty(B, L, dtype=torch.uint8, device=dev)
    keys = torch.empty(B, cap, dtype=torch.int64, device=dev)
    n_min, n_anchors, truncated = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    result = torch.empty(B, 8, dtype=torch.int32, device=dev)
    f, pred = (torch.empty(B, cap, dtype=torch.int32, device=dev) for _ in range(2))
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    c = DEFAULTS

    def sketch():
        _lib.check(lib.wn_minimizers(_p(labels), labels.stride(0), _p(lengths), B, L, k, w, 0, _p(code), _p(flag), _p(bad), _stream()), "wn_minimizers")

    def seeds():
        _lib.check(lib.wn_read_seeds(_p(code), _p(flag), _p(lengths), _p(index.entries), index.n_entries, B, L, k, max_occ, cap, _p(keys),
                                     _p(n_min), _p(n_anchors), _p(truncated), _p(bad), _stream()), "wn_read_seeds")

    def chain(table=False):
        _lib.check(lib.wn_chain(_p(keys), _p(n_anchors), _p(lengths), B, L, cap, k, c["h"], c["max_dist"], c["bandwidth"], c["gap_base"],
                                c["gap_log"], _p(result), _p(f) if table else None, _p(pred) if table else None, _p(bad), _stream()), "wn_chain")

    sketch()
    seeds()
    chain(True)
    torch.cuda.synchronize()
    assert int(bad[0]) == 0
    anchors, minimizers = int(n_anchors.sum()), int(n_min.sum())
    pairs = pairs_evaluated(keys, n_anchors, c["h"])
    whole = W.map_reads(labels, lengths, index, want_pred=True)
    assert torch.equal(torch.stack(list(whole[:8]), 1), result) and torch.equal(whole.f, f) and torch.equal(whole.pred, pred)
    assert torch.equal(whole.anchors.keys, keys) and torch.equal(torch.sort(keys, dim=1).values, keys)          # the rows come sorted
    mapped = int(whole.mapped.sum())
    rep = Report()
    lines = ["# read mapping: %d reads of 400..1200 labels (8 %% errors, both strands; rows of %d) against %d bases, k %d w %d max_occ %d h %d, "
             "%d anchors per read at most, %s" % (B, L, a.reference, k, w, max_occ, c["h"], cap, torch.cuda.get_device_name(0)),
             "# index: %d entries, built in %.1f ms (first call %.1f ms); reads: %d minimizers, %d anchors (%.1f per read, %d reads truncated), "
             "%d predecessor pairs, %d reads mapped" % (index.n_entries, index_ms2, index_ms, minimizers, anchors, anchors / B,
                                                        int(truncated.sum()), pairs, mapped),
             "%-28s %10s %10s %10s %6s" % ("stage", "median ms", "least", "greatest", "reps")]
    for line in lines:
        rep.emit(line)
    times = {}
    for name, fn in (("sketch (wn_minimizers)", sketch), ("seeds, sorted (wn_read_seeds)", seeds), ("chain (wn_chain)", chain),
                     ("chain with f and pred", lambda: chain(True)), ("map_reads (python, all three)", lambda: W.map_reads(labels, lengths, index))):
        t = timed(fn, calls=a.reps, windows=a.repeats, warmup=a.warmup, min_seconds=a.min_seconds)
        times[name] = t.median
        rep.emit("%-28s %10.4f %10.4f %10.4f %6d" % (name, t.median, t.least, t.greatest, t.calls))
    t = times["chain (wn_chain)"] * 1e-3
    rep.emit("chain: %.3g anchors/s, %.3g predecessor pairs/s; all three stages: %.3g reads/s" % (
        anchors / t, pairs / t, B / (1e-3 * sum(times[n] for n in list(times)[:3]))))
    if not a.no_torch:
        tf, tp = torch_chain(keys, n_anchors, k, **c)
        assert torch.equal(tf, f) and torch.equal(tp, pred), "the comparator's chain table differs from the kernel's"
        t = timed(lambda: torch_chain(keys, n_anchors, k, **c), windows=min(a.repeats, 3), warmup=1)
        rep.emit("%-28s %10.4f %10.4f %10.4f %6d   (%.0fx the kernel with the table)" % ("torch-op chain DP", t.median, t.least, t.greatest,
                                                                                        t.calls, t.median / times["chain with f and pred"]))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
