#!/usr/bin/env python3
"""Time the pileup and the consensus calls (csrc/wn_pileup.hip: wn_pileup, wn_consensus_call, wn_consensus_emit) on the GPU at the
shape of a bacterial run: 4096 reads of 1600..2400 op columns (about 2000 bases; 3 % mismatches, 3 % deletions, 4 % insertions in
runs, eight end columns on either side, both strands) laid on random windows of a reference of 4.6 M bases.  The op strings are
drawn directly -- they are what pairwise_align writes, and aligning 4096 such pairs is another tool's time.

What is timed.  wn_pileup through the C ABI on preallocated tables (the kernel and its launch, nothing else), pileup() and
call_consensus() through the Python surface (with their allocations; call_consensus with its one read-back); device events around
`reps` calls after `warmup` calls, reps raised until the window is at least --min-seconds; every window is taken --repeats times
and the median is reported with the least and the greatest.

The comparator.  The same three tables from torch ops on the same GPU: the reverse-strand rows turned round by a gather, cumsum
over the op columns for the reference / query index, cummax for the last column that is no insertion, then three
index_put_(accumulate=True).  It is written for this tool only and is not shipped; its tables must equal the kernel's exactly
before any time is printed.
Usage: pileup_bench.py [--reads N] [--reference N] [--reps N] [--warmup N] [--min-seconds S] [--repeats N] [--no-torch] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gputime import Report, timed  # noqa: E402


def make_reads(rng, count, reference, lo=1600, hi=2400):
    """(ops [count, width] uint8, ops_len, window lo, ref_lengths, strand, query [count, M] int32, query_lengths)"""
    rows, queries = [], []
    for b in range(count):
        n = int(rng.integers(lo, hi + 1))
        u = rng.random(n)
        ops = np.where(u < 0.90, 1, np.where(u < 0.93, 2, np.where(u < 0.96, 3, 4))).astype(np.uint8)
        ops[(ops == 4) & (np.roll(ops, 1) == 4) & (rng.random(n) < 0.5)] = 1          # fewer, not only single, insertion columns
        grow = np.flatnonzero((ops == 4) & (rng.random(n) < 0.3))
        ops[np.minimum(grow + 1, n - 1)] = 4
        ops[:8], ops[-8:] = 3, 3                                                         # the flank of the window: end columns
        ops[8], ops[-9] = 1, 1
        rows.append(ops)
        queries.append(rng.integers(1, 5, int((ops != 3).sum())).astype(np.int32))
    width, M = max(len(r) for r in rows), max(len(q) for q in queries)
    ops, query = np.zeros((count, width), dtype=np.uint8), np.zeros((count, M), dtype=np.int32)
    for b in range(count):
        ops[b, :len(rows[b])], query[b, :len(queries[b])] = rows[b], queries[b]
    ref_len = np.array([int((r != 4).sum()) for r in rows], dtype=np.int32)
    start = np.array([int(rng.integers(0, reference - n + 1)) for n in ref_len], dtype=np.int32)
    return (ops, np.array([len(r) for r in rows], dtype=np.int32), start, ref_len, (np.arange(count) & 1).astype(np.int32), query,
            np.array([len(q) for q in queries], dtype=np.int32))


def torch_pileup(ops, ops_len, lo, ref_len, strand, query, query_len, R, max_ins):
    """the three tables by torch ops: (counts [R, 2, 6], ins_lengths [R, max_ins + 1], ins_bases [R, max_ins, 4]) int32"""
    dev = ops.device
    B, width = ops.shape
    c = torch.arange(width, device=dev)[None, :]
    n, rev = ops_len[:, None].long(), (strand == 1)[:, None]
    live = c < n
    op = torch.where(live, ops.gather(1, torch.where(rev, n - 1 - c, c).clamp(0, width - 1)).long(), torch.zeros_like(c))       # walk order
    is_ref, is_query, non4 = (op >= 1) & (op <= 3), (op == 1) | (op == 2) | (op == 4), live & (op != 4)
    i, j = torch.cumsum(is_ref, 1) - is_ref.long(), torch.cumsum(is_query, 1) - is_query.long()
    aligned = (op == 1) | (op == 2)
    first = torch.where(aligned, c, torch.full_like(c, width)).min(1, keepdim=True).values
    last = torch.where(aligned, c, torch.full_like(c, -1)).max(1, keepdim=True).values
    inside = live & (c >= first) & (c <= last)
    last_non4 = torch.cummax(torch.where(non4, c, torch.full_like(c, -1)), 1).values
    prev = torch.cat([torch.full((B, 1), -1, device=dev, dtype=torch.long), last_non4[:, :-1]], 1)       # strictly before the column
    jq = torch.where(rev, query_len[:, None].long() - 1 - j, j).clamp(0, query.shape[1] - 1)
    label = query.gather(1, jq).long()
    base_ok = (label >= 1) & (label <= 4)
    base = torch.where(rev, 4 - label, label - 1)
    s = strand[:, None].long().expand(B, width)
    counts = torch.zeros(R * 12, dtype=torch.int32, device=dev)
    ins_lengths = torch.zeros(R * (max_ins + 1), dtype=torch.int32, device=dev)
    ins_bases = torch.zeros(R * max_ins * 4, dtype=torch.int32, device=dev)
    pos = lo[:, None].long() + i
    one = torch.ones(1, dtype=torch.int32, device=dev)
    sel = inside & (op != 4)
    col = torch.where(op == 3, torch.full_like(op, 4), torch.where(base_ok, base, torch.full_like(op, 5)))
    counts.index_put_((((pos * 2 + s) * 6 + col)[sel],), one, accumulate=True)
    sel = sel & (c > first) & (prev != c - 1)                                            # the column after an insertion run
    length = (c - 1 - prev).clamp(max=max_ins + 1)
    ins_lengths.index_put_((((pos - 1) * (max_ins + 1) + length - 1)[sel],), one, accumulate=True)
    k = c - prev - 1
    sel = inside & (op == 4) & (k < max_ins) & base_ok
    ins_bases.index_put_(((((pos - 1) * max_ins + k) * 4 + base)[sel],), one, accumulate=True)
    return counts.view(R, 2, 6), ins_lengths.view(R, max_ins + 1), ins_bases.view(R, max_ins, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--reference", type=int, default=4600000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-op comparator")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "pileup_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pileup_bench.py measures the GPU; there is no CPU path"
    import wavenet_speech_amd as W
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(47)
    R, max_ins = a.reference, 4
    host = make_reads(rng, a.reads, R)
    ops, ops_len, lo, ref_len, strand, query, query_len = (torch.from_numpy(x).to(dev) for x in host)
    reference = torch.from_numpy(rng.integers(1, 5, R).astype(np.int32)).to(dev)
    B, width, M = ops.shape[0], ops.shape[1], query.shape[1]
    aln = W.PairwiseAlignment(None, None, None, None, None, ops, ops_len)
    counts = torch.zeros(R, 2, 6, dtype=torch.int32, device=dev)
    ins_lengths = torch.zeros(R, max_ins + 1, dtype=torch.int32, device=dev)
    ins_bases = torch.zeros(R, max_ins, 4, dtype=torch.int32, device=dev)
    used = torch.empty(B, dtype=torch.int8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def kernel():
        _lib.check(lib.wn_pileup(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_len), _p(strand), _p(query), query.stride(0), _p(query_len),
                                 None, 0, None, B, M, width, R, 0, max_ins, _p(counts), _p(ins_lengths), _p(ins_bases), _p(used), _p(bad),
                                 _stream()), "wn_pileup")

    kernel()
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and int((used != 1).sum()) == 0
    pile = W.pileup(aln, lo, ref_len, strand, query, query_len, R, max_ins=max_ins)
    assert torch.equal(pile.counts, counts) and torch.equal(pile.ins_lengths, ins_lengths) and torch.equal(pile.ins_bases, ins_bases)
    columns, adds = int(ops_len.sum()), int(counts.sum()) + int(ins_lengths.sum()) + int(ins_bases.sum())
    calls = W.call_consensus(pile, reference)
    rep = Report()
    lines = ["# pileup: %d reads of %d..%d op columns (rows of %d; queries of at most %d) on a reference of %d, max_ins %d, both strands, %s"
             % (B, int(ops_len.min()), int(ops_len.max()), width, M, R, max_ins, torch.cuda.get_device_name(0)),
             "# %d op columns, %d atomic adds; mean depth over the reference %.2f; consensus of %d labels, %d positions called"
             % (columns, adds, float(pile.depth.double().mean()), int(calls.consensus.shape[0]), int((calls.flags & 28 != 0).sum())),
             "%-34s %10s %10s %10s %6s" % ("stage", "median ms", "least", "greatest", "reps")]
    for line in lines:
        rep.emit(line)
    times = {}
    for name, fn in (("pileup (wn_pileup)", kernel),
                     ("pileup (python, fresh tables)", lambda: W.pileup(aln, lo, ref_len, strand, query, query_len, R, max_ins=max_ins)),
                     ("pileup (python, into=)", lambda: W.pileup(aln, lo, ref_len, strand, query, query_len, R, max_ins=max_ins, into=pile)),
                     ("call_consensus (python, 3 launches)", lambda: W.call_consensus(pile, reference))):
        t = timed(fn, calls=a.reps, windows=a.repeats, warmup=a.warmup, min_seconds=a.min_seconds)
        times[name] = t.median
        rep.emit("%-34s %10.4f %10.4f %10.4f %6d" % (name, t.median, t.least, t.greatest, t.calls))
    t = times["pileup (wn_pileup)"] * 1e-3
    rep.emit("pileup: %.3g op columns/s, %.3g reads/s; call_consensus: %.3g positions/s" % (
        columns / t, B / t, R / (1e-3 * times["call_consensus (python, 3 launches)"])))
    if not a.no_torch:
        fresh = W.pileup(aln, lo, ref_len, strand, query, query_len, R, max_ins=max_ins)
        tc, tl, tb = torch_pileup(ops, ops_len, lo, ref_len, strand, query, query_len, R, max_ins)
        assert torch.equal(tc, fresh.counts) and torch.equal(tl, fresh.ins_lengths) and torch.equal(tb, fresh.ins_bases), \
            "the comparator's tables differ from the kernel's"
        t = timed(lambda: torch_pileup(ops, ops_len, lo, ref_len, strand, query, query_len, R, max_ins), calls=2, windows=min(a.repeats, 3),
                  warmup=1)
        rep.emit("%-34s %10.4f %10.4f %10.4f %6d   (%.1fx pileup (python, fresh tables))" % (
            "torch-op pileup (fresh tables)", t.median, t.least, t.greatest, t.calls, t.median / times["pileup (python, fresh tables)"]))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
