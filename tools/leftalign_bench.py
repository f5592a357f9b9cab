#!/usr/bin/env python3
"""Time the indel left-alignment (csrc/wn_leftalign.hip: wn_gap_left_align) on the GPU on the op strings of tools/pileup_bench.py:
4096 reads of 1600..2400 op columns (3 % mismatches, 3 % deletions, 4 % insertions in runs, eight end columns on either side, both
strands).  The labels are drawn to fit the ops: a random window, the read derived from it column by column (op 1 copies the label,
op 2 changes it, op 4 inserts one), and -- for the share --repeat-share of the gap runs -- a homopolymer of 3 to 12 labels laid to
either side of the run (mismatch columns break it), so that the run has somewhere to go on either strand.  How many rows changed,
the passes they took and the columns that differ are counted from the result and printed: the share is what was asked for, those
are what came (random labels alone let a run move one column in four).

What is timed.  wn_gap_left_align through the C ABI into a preallocated row block (the kernel and its launch, nothing else) and
left_align() through the Python surface (with its allocations), beside wn_pileup through the C ABI on the same strings in the same
process; device events around `reps` calls after `warmup` calls, reps raised until the window is at least --min-seconds; every
window is taken --repeats times and the median is reported with the least and the greatest.  No speed is asserted.
Usage: leftalign_bench.py [--reads N] [--repeat-share F] [--max-passes N] [--reps N] [--warmup N] [--min-seconds S] [--repeats N] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gputime import Report, timed  # noqa: E402
from pileup_bench import make_reads  # noqa: E402


def make_labels(rng, ops, share):
    """(a, b) int32 label arrays that fit one op row (read orientation), a homopolymer around `share` of the gap runs"""
    n_ref, n_query = int((ops != 4).sum()), int((ops != 3).sum())
    a = rng.integers(1, 5, n_ref).astype(np.int32)
    i_at = np.cumsum(ops != 4) - (ops != 4)
    j_at = np.cumsum(ops != 3) - (ops != 3)
    gap = ops >= 3
    starts = np.flatnonzero(gap & ~np.concatenate([[False], (ops[1:] == ops[:-1])]))
    chosen = starts[rng.random(len(starts)) < share]
    for c in chosen:                                                 # the window around the run: one label, k to either side
        e = c
        while e < len(ops) and ops[e] == ops[c]:
            e += 1
        x, k = int(i_at[c]), int(rng.integers(3, 13))
        hi = x + (e - c if ops[c] == 3 else 0)
        a[max(x - k, 0):hi + k] = a[min(x, n_ref - 1)]
    b = np.zeros(n_query, dtype=np.int32)
    aligned = ops <= 2
    b[j_at[aligned]] = a[i_at[aligned]]
    wrong = ops == 2
    b[j_at[wrong]] = (a[i_at[wrong]] - 1 + rng.integers(1, 4, int(wrong.sum()))) % 4 + 1
    b[j_at[ops == 4]] = rng.integers(1, 5, int((ops == 4).sum()))
    for c in chosen[ops[chosen] == 4]:                               # an insertion repeats that label
        e = c
        while e < len(ops) and ops[e] == 4:
            e += 1
        b[int(j_at[c]):int(j_at[c]) + (e - c)] = a[min(int(i_at[c]), n_ref - 1)]
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--repeat-share", type=float, default=0.3)
    ap.add_argument("--max-passes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "leftalign_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "leftalign_bench.py measures the GPU; there is no CPU path"
    import wavenet_speech_amd as W
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(47)
    R, max_ins = 4600000, 4
    h_ops, h_len, h_lo, h_ref_len, h_strand, _, h_query_len = make_reads(rng, a.reads, R)
    B, width = h_ops.shape
    N, M = int(h_ref_len.max()), int(h_query_len.max())
    h_ref, h_query = np.zeros((B, N), dtype=np.int32), np.zeros((B, M), dtype=np.int32)
    for r in range(B):
        # aligned columns 1 / 2 must agree with the labels; the mismatch rule of make_labels keeps them so
        ra, rb = make_labels(rng, h_ops[r, :h_len[r]], a.repeat_share)
        h_ref[r, :len(ra)], h_query[r, :len(rb)] = ra, rb
    ops, ops_len, lo, ref_len, strand, query_len, ref, query = (torch.from_numpy(x).to(dev) for x in (h_ops, h_len, h_lo, h_ref_len, h_strand,
                                                                                                   h_query_len, h_ref, h_query))
    aln = W.PairwiseAlignment(None, None, None, None, None, ops, ops_len)
    out = torch.empty_like(ops)
    passes, settled = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.zeros(R, 2, 6, dtype=torch.int32, device=dev)
    ins_lengths = torch.zeros(R, max_ins + 1, dtype=torch.int32, device=dev)
    ins_bases = torch.zeros(R, max_ins, 4, dtype=torch.int32, device=dev)
    used = torch.empty(B, dtype=torch.int8, device=dev)

    def kernel():
        _lib.check(lib.wn_gap_left_align(_p(ops), ops.stride(0), _p(ops_len), _p(ref), ref.stride(0), _p(ref_len), _p(query), query.stride(0),
                                         _p(query_len), _p(strand), B, N, M, width, a.max_passes, _p(out), out.stride(0), _p(passes), _p(settled),
                                         None, 0, _p(bad), _stream()), "wn_gap_left_align")

    def pileup_kernel():
        _lib.check(lib.wn_pileup(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_len), _p(strand), _p(query), query.stride(0), _p(query_len),
                                 None, 0, None, B, M, width, R, 0, max_ins, _p(counts), _p(ins_lengths), _p(ins_bases), _p(used), _p(bad),
                                 _stream()), "wn_pileup")

    kernel()
    pileup_kernel()
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and int((settled < 0).sum()) == 0 and int((used != 1).sum()) == 0
    la = W.left_align(aln, ref, ref_len, query, query_len, strand, max_passes=a.max_passes)
    assert torch.equal(la.alignment.ops, out) and torch.equal(la.passes, passes)
    interior = (ops >= 3)
    runs = int((interior & ~torch.cat([torch.zeros(B, 1, dtype=torch.bool, device=dev), ops[:, 1:] == ops[:, :-1]], 1)).sum())
    rep = Report()
    lines = ["# left_align: %d reads of %d..%d op columns (rows of %d), windows of at most %d and reads of at most %d labels, both strands, "
             "max_passes %d, %s" % (B, int(ops_len.min()), int(ops_len.max()), width, N, M, a.max_passes, torch.cuda.get_device_name(0)),
             "# %d op columns, %d gap runs, a homopolymer asked for around %.0f %% of them; %d rows changed, passes per row mean %.2f "
             "max %d, %d rows not settled, %d columns differ" % (int(ops_len.sum()), runs, 100 * a.repeat_share, int((passes > 0).sum()),
                                                                float(passes.float().mean()), int(passes.max()), int((settled == 0).sum()),
                                                                int((out != ops).sum())),
             "%-34s %10s %10s %10s %6s" % ("stage", "median ms", "least", "greatest", "reps")]
    for line in lines:
        rep.emit(line)
    times = {}
    for name, fn in (("left_align (wn_gap_left_align)", kernel),
                     ("left_align (python)", lambda: W.left_align(aln, ref, ref_len, query, query_len, strand, max_passes=a.max_passes)),
                     ("pileup (wn_pileup)", pileup_kernel)):
        t = timed(fn, calls=a.reps, windows=a.repeats, warmup=a.warmup, min_seconds=a.min_seconds)
        times[name] = t.median
        rep.emit("%-34s %10.4f %10.4f %10.4f %6d" % (name, t.median, t.least, t.greatest, t.calls))
    t = times["left_align (wn_gap_left_align)"] * 1e-3
    rep.emit("left_align: %.3g op columns/s, %.3g reads/s; %.2fx the time of wn_pileup on the same strings" % (
        int(ops_len.sum()) / t, B / t, times["left_align (wn_gap_left_align)"] / times["pileup (wn_pileup)"]))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
