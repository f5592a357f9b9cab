#!/usr/bin/env python3
"""Time the genotype evidence and the diploid calls (csrc/wn_genotype.hip: wn_pileup_evidence, wn_genotype_call) on the GPU on the
reads of tools/pileup_bench.py: 4096 reads of 1600..2400 op columns (3 % mismatches, 3 % deletions, 4 % insertions in runs, eight
end columns on either side, both strands) on random windows of a reference of 4.6 M bases, with random quals 0..40.

What is timed.  wn_pileup_evidence through the C ABI on a preallocated table beside wn_pileup through the C ABI on the same reads
in the same process -- the same walk with one 32-bit add per column where the new kernel makes three 64-bit adds -- once without
and once with quals; pileup_evidence() and call_genotypes() through the Python surface (with their allocations) beside
call_consensus() (three launches and its one read-back).  Device events around `reps` calls after `warmup` calls, reps raised until
the window is at least --min-seconds; every window is taken --repeats times and the median is reported with the least and the
greatest.  Before any time is printed, the evidence under a table of ones must equal the counts of wn_pileup.  No speed is asserted.
Usage: genotype_bench.py [--reads N] [--reference N] [--reps N] [--warmup N] [--min-seconds S] [--repeats N] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--reference", type=int, default=4600000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "genotype_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "genotype_bench.py measures the GPU; there is no CPU path"
    import wavenet_speech_amd as W
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(47)
    R, max_ins = a.reference, 4
    host = make_reads(rng, a.reads, R)
    ops, ops_len, lo, ref_len, strand, query, query_len = (torch.from_numpy(x).to(dev) for x in host)
    qual = torch.from_numpy(rng.integers(0, 41, size=host[5].shape).astype(np.uint8)).to(dev)
    reference = torch.from_numpy(rng.integers(1, 5, R).astype(np.int32)).to(dev)
    B, width, M = ops.shape[0], ops.shape[1], query.shape[1]
    aln = W.PairwiseAlignment(None, None, None, None, None, ops, ops_len)
    weights = W.genotype_weights()
    table = weights.checked("genotype_bench")
    counts = torch.zeros(R, 2, 6, dtype=torch.int32, device=dev)
    ins_lengths = torch.zeros(R, max_ins + 1, dtype=torch.int32, device=dev)
    ins_bases = torch.zeros(R, max_ins, 4, dtype=torch.int32, device=dev)
    evidence = torch.zeros(R, 5, 3, dtype=torch.int64, device=dev)
    used = torch.empty(B, dtype=torch.int8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def pile_kernel(q=None):
        _lib.check(lib.wn_pileup(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_len), _p(strand), _p(query), query.stride(0), _p(query_len),
                                 _p(q), q.stride(0) if q is not None else 0, None, B, M, width, R, 7 if q is not None else 0, max_ins, _p(counts),
                                 _p(ins_lengths), _p(ins_bases), _p(used), _p(bad), _stream()), "wn_pileup")

    def evidence_kernel(q=None, t=table, into=evidence):
        _lib.check(lib.wn_pileup_evidence(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_len), _p(strand), _p(query), query.stride(0),
                                          _p(query_len), _p(q), q.stride(0) if q is not None else 0, None, B, M, width, R, None,
                                          ctypes.cast(t, ctypes.c_void_p), 20, 20, 7 if q is not None else 0, _p(into), _p(used), _p(bad),
                                          _stream()), "wn_pileup_evidence")

    # the two walks pick the same columns: under a table of ones every cell is the count over both strands
    pile_kernel(qual)
    ones = torch.zeros_like(evidence)
    evidence_kernel(qual, (ctypes.c_int * (3 * 94))(*([1] * (3 * 94))), ones)
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and int((used != 1).sum()) == 0
    assert torch.equal(ones, counts[:, :, :5].sum(1).long()[:, :, None].expand(R, 5, 3)), "the evidence walk differs from the pileup's"
    del ones
    counts.zero_(), ins_lengths.zero_(), ins_bases.zero_()
    pile = W.pileup(aln, lo, ref_len, strand, query, query_len, R, qual=qual, min_qual=7, max_ins=max_ins)
    ev = W.pileup_evidence(aln, lo, ref_len, strand, query, query_len, R, weights, qual=qual, min_qual=7)
    calls = W.call_genotypes(pile, ev, reference, weights)
    columns = int(ops_len.sum())
    rep = Report()
    lines = ["# genotype: %d reads of %d..%d op columns (rows of %d; queries of at most %d) on a reference of %d, both strands, quals 0..40, %s"
             % (B, int(ops_len.min()), int(ops_len.max()), width, M, R, torch.cuda.get_device_name(0)),
             "# %d op columns, %d evidence cells added into (3 atomics each); mean depth %.2f; %d positions with a variant flag, %d heterozygous"
             % (columns, int(pile.counts[:, :, :5].sum()), float(pile.depth.double().mean()), int((calls.flags & 28 != 0).sum()),
                int((calls.flags & 32 != 0).sum())),
             "%-44s %10s %10s %10s %6s" % ("stage", "median ms", "least", "greatest", "reps")]
    for line in lines:
        rep.emit(line)
    times = {}
    for name, fn in (("pileup (wn_pileup, no qual)", pile_kernel),
                     ("evidence (wn_pileup_evidence, no qual)", evidence_kernel),
                     ("pileup (wn_pileup, qual)", lambda: pile_kernel(qual)),
                     ("evidence (wn_pileup_evidence, qual)", lambda: evidence_kernel(qual)),
                     ("pileup_evidence (python, fresh table)", lambda: W.pileup_evidence(aln, lo, ref_len, strand, query, query_len, R, weights,
                                                                                        qual=qual, min_qual=7)),
                     ("pileup_evidence (python, into=)", lambda: W.pileup_evidence(aln, lo, ref_len, strand, query, query_len, R, weights, qual=qual,
                                                                                  min_qual=7, into=ev)),
                     ("call_consensus (python, 3 launches)", lambda: W.call_consensus(pile, reference)),
                     ("call_genotypes (python, 1 launch)", lambda: W.call_genotypes(pile, ev, reference, weights)),
                     ("call_genotypes (python, with costs)", lambda: W.call_genotypes(pile, ev, reference, weights, return_costs=True))):
        t = timed(fn, calls=a.reps, windows=a.repeats, warmup=a.warmup, min_seconds=a.min_seconds)
        times[name] = t.median
        rep.emit("%-44s %10.4f %10.4f %10.4f %6d" % (name, t.median, t.least, t.greatest, t.calls))
    rep.emit("evidence / pileup: %.2fx without qual, %.2fx with; evidence: %.3g op columns/s; call_genotypes / call_consensus: %.2fx, %.3g positions/s" % (
        times["evidence (wn_pileup_evidence, no qual)"] / times["pileup (wn_pileup, no qual)"],
        times["evidence (wn_pileup_evidence, qual)"] / times["pileup (wn_pileup, qual)"],
        columns / (1e-3 * times["evidence (wn_pileup_evidence, qual)"]),
        times["call_genotypes (python, 1 launch)"] / times["call_consensus (python, 3 launches)"],
        R / (1e-3 * times["call_genotypes (python, 1 launch)"])))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
