#!/usr/bin/env python3
"""Time the two kernels around the realignment DP (csrc/wn_realign.hip: wn_haplotype_windows, wn_lift_ops) on the GPU on the reads of
tools/pileup_bench.py: 4096 reads of 1600..2400 op columns (3 % mismatches, 3 % deletions, 4 % insertions in runs, both strands) on
random windows of a reference of 4.6 M bases.  Those reads are random labels, not a diploid sample, so both inputs are PLANTED:
  windows  two haplotypes over the whole reference that differ from it by a substitution, a deleted position or an insertion of
           1..4 labels at one position in --edit-every (500) each; the windows are the reads' own.
  lift     A is the read's op row of tools/pileup_bench.py taken as the read against the HAPLOTYPE (its reference labels are the
           haplotype's), Hh a row that holds as many haplotype labels with a 3 or a 4 at one column in --edit-every; the reference
           window is what Hh consumes.  Both rows are valid, so every read composes.

What is timed.  The two entry points through the C ABI on preallocated outputs beside wn_pileup_evidence through the C ABI on the
same reads in the same process (the walk every read tool shares: two passes over the op row and three 64-bit adds per column), and
haplotype_windows / lift_alignment through the Python surface with their allocations.  Device events around `reps` calls after
`warmup` calls, reps raised until the window is at least --min-seconds; every window is taken --repeats times and the median is
reported with the least and the greatest (tools/gputime.py, DESIGN.md section 7q's protocol).  Before any time is printed no read
may be bad and every lifted row must consume exactly its window and its read.  No speed is asserted.
Usage: realign_bench.py [--reads N] [--reference N] [--edit-every N] [--reps N] [--warmup N] [--min-seconds S] [--repeats N] [--out FILE]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gputime import Report, timed  # noqa: E402
from pileup_bench import make_reads  # noqa: E402


def planted_haplotypes(rng, reference, every, max_ins):
    R = len(reference)
    call = np.tile(reference.astype(np.uint8), (2, 1))
    ins_len = np.zeros((2, R), dtype=np.uint8)
    ins_bases = np.zeros((2, R, max_ins), dtype=np.uint8)
    for h in range(2):
        u = rng.random(R) * every
        call[h][u < 1] = rng.integers(1, 5, size=int((u < 1).sum()))
        call[h][(u >= 1) & (u < 2)] = 0
        at = np.flatnonzero((u >= 2) & (u < 3))
        ins_len[h][at] = rng.integers(1, max_ins + 1, size=len(at))
        ins_bases[h][at] = rng.integers(1, 5, size=(len(at), max_ins))
    return call, ins_len, ins_bases


def haplotype_rows(rng, hap_len, every):
    """Hh rows that hold hap_len[b] haplotype labels: ones with a 3 put in or a label turned into a 4 at one column in `every`"""
    rows = []
    for n in hap_len:
        row = np.ones(int(n), dtype=np.uint8)
        row[rng.random(int(n)) * every < 1] = 4
        rows.append(np.insert(row, np.sort(rng.integers(0, int(n) + 1, size=max(1, int(n) // every))), 3))
    width = max(len(r) for r in rows)
    out = np.zeros((len(rows), width), dtype=np.uint8)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, np.array([len(r) for r in rows], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--reference", type=int, default=4600000)
    ap.add_argument("--edit-every", type=int, default=500)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "realign_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "realign_bench.py measures the GPU; there is no CPU path"
    import wavenet_speech_amd as W
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(53)
    R, max_ins = a.reference, 4
    host = make_reads(rng, a.reads, R)
    ops, ops_len, lo, ref_len, strand, query, query_len = (torch.from_numpy(x).to(dev) for x in host)
    B, width, M = ops.shape[0], ops.shape[1], query.shape[1]
    on = lambda x: torch.from_numpy(x).to(dev)                       # noqa: E731

    # ---- the windows: planted haplotypes over the reference, the reads' own windows
    reference = rng.integers(1, 5, size=R).astype(np.int32)
    hcalls = W.HaplotypeCalls(*(on(x) for x in planted_haplotypes(rng, reference, a.edit_every, max_ins)))
    reference = on(reference)
    cap = int(host[3].max()) + 64
    labels = torch.empty(2, B, cap, dtype=torch.int32, device=dev)
    hap_ops = torch.empty(2, B, cap, dtype=torch.uint8, device=dev)
    lengths, hap_ops_len = (torch.empty(2, B, dtype=torch.int32, device=dev) for _ in range(2))
    used = torch.empty(B, dtype=torch.int8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def windows_kernel():
        _lib.check(lib.wn_haplotype_windows(_p(hcalls.call), _p(hcalls.ins_len), _p(hcalls.ins_bases), _p(reference), _p(lo), _p(ref_len), _p(strand),
                                            2, B, R, max_ins, cap, _p(labels), _p(lengths), _p(hap_ops), _p(hap_ops_len), _p(used), _p(bad), _stream()),
                   "wn_haplotype_windows")

    windows_kernel()
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and int((used != 1).sum()) == 0, "a window did not fit"
    window_ops = int(hap_ops_len.sum())

    # ---- the lift: the reads' op rows as A, planted Hh rows with as many haplotype labels
    hh, hh_len = haplotype_rows(rng, host[3], a.edit_every)
    lift_ref_len = on((hh != 4).sum(1).astype(np.int32) - (hh.shape[1] - hh_len))       # the padding is not a column
    N = int(lift_ref_len.max())
    lift_ref = on(rng.integers(1, 5, size=(B, N)).astype(np.int32))
    hh, hh_len = on(hh), on(hh_len)
    windows = W.HaplotypeWindows(None, ref_len.reshape(1, B), hh.unsqueeze(0), hh_len.reshape(1, B), torch.ones(B, dtype=torch.int8, device=dev))
    pick = torch.zeros(B, dtype=torch.int32, device=dev)
    max_ops = N + M
    out = torch.empty(B, max_ops, dtype=torch.uint8, device=dev)
    out_len, score = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    stats = torch.empty(B, 4, dtype=torch.int32, device=dev)
    ws_bytes = lib.wn_lift_ops_workspace_bytes(B, hh.shape[1])
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def lift_kernel():
        _lib.check(lib.wn_lift_ops(_p(ops), 0, ops.stride(0), _p(ops_len), width, _p(hh), 0, hh.stride(0), _p(hh_len), _p(ref_len), hh.shape[1],
                                   hh.shape[1], _p(windows.used), _p(pick), _p(lift_ref), lift_ref.stride(0), _p(lift_ref_len), _p(query),
                                   query.stride(0), _p(query_len), 1, B, N, M, max_ops, 10, -8, 20, 1, 1, _p(out), out.stride(0), _p(out_len),
                                   _p(score), _p(stats), _p(ws), ws_bytes, _p(bad), _stream()), "wn_lift_ops")

    lift_kernel()
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and int((out_len <= 0).sum()) == 0, "a read did not compose"
    live = torch.arange(max_ops, device=dev)[None, :] < out_len[:, None]
    assert torch.equal(((out != 4) & live).sum(1).int(), lift_ref_len) and torch.equal(((out != 3) & live).sum(1).int(), query_len), \
        "a lifted row does not consume its window and its read"
    aln = W.PairwiseAlignment(None, None, None, None, None, ops, ops_len)

    # ---- the walk every read tool shares, on the same reads
    table = W.genotype_weights().checked("realign_bench")
    evidence = torch.zeros(R, 5, 3, dtype=torch.int64, device=dev)

    def evidence_kernel():
        _lib.check(lib.wn_pileup_evidence(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_len), _p(strand), _p(query), query.stride(0),
                                          _p(query_len), None, 0, None, B, M, width, R, None, ctypes.cast(table, ctypes.c_void_p), 20, 20, 0,
                                          _p(evidence), _p(used), _p(bad), _stream()), "wn_pileup_evidence")

    rep = Report()
    for line in ("# realign: %d reads of %d..%d op columns (rows of %d; queries of at most %d) on a reference of %d, both strands, %s"
                 % (B, int(ops_len.min()), int(ops_len.max()), width, M, R, torch.cuda.get_device_name(0)),
                 "# windows: 2 haplotypes, %d op columns written in rows of %d; lift: %d + %d op columns read, %d written, workspace %.1f MB"
                 % (window_ops, cap, int(ops_len.sum()), int(hh_len.sum()), int(out_len.sum()), ws_bytes / 1e6),
                 "%-52s %10s %10s %10s %6s" % ("stage", "median ms", "least", "greatest", "reps")):
        rep.emit(line)
    times = {}
    for name, fn in (("evidence (wn_pileup_evidence, no qual)", evidence_kernel),
                     ("windows (wn_haplotype_windows, 2 haplotypes)", windows_kernel),
                     ("lift (wn_lift_ops)", lift_kernel),
                     ("haplotype_windows (python, fresh tables)", lambda: W.haplotype_windows(hcalls, reference, lo, ref_len, strand, max_hap_ops=cap)),
                     ("lift_alignment (python, fresh tables)", lambda: W.lift_alignment(aln, windows, pick, lift_ref, lift_ref_len, query, query_len))):
        t = timed(fn, calls=a.reps, windows=a.repeats, warmup=a.warmup, min_seconds=a.min_seconds)
        times[name] = t.median
        rep.emit("%-52s %10.4f %10.4f %10.4f %6d" % (name, t.median, t.least, t.greatest, t.calls))
    rep.emit("windows / evidence: %.2fx; lift / evidence: %.2fx; windows: %.3g op columns/s; lift: %.3g op columns/s" % (
        times["windows (wn_haplotype_windows, 2 haplotypes)"] / times["evidence (wn_pileup_evidence, no qual)"],
        times["lift (wn_lift_ops)"] / times["evidence (wn_pileup_evidence, no qual)"],
        window_ops / (1e-3 * times["windows (wn_haplotype_windows, 2 haplotypes)"]), int(out_len.sum()) / (1e-3 * times["lift (wn_lift_ops)"])))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
