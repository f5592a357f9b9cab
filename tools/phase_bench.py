#!/usr/bin/env python3
"""Time the phasing step (csrc/wn_phase.hip: wn_phase_links, wn_phase_chain, wn_haplotag) on the GPU on the reads of
tools/pileup_bench.py: 4096 reads of 1600..2400 op columns (3 % mismatches, 3 % deletions, 4 % insertions in runs, eight end columns
on either side, both strands) on random windows of a reference of 4.6 M bases, with random quals 0..40.  Those reads are random
labels, not a diploid sample, so the sites are PLANTED: every position is a site with chance 1 / --site-every (500: about four per
read), with two different random alleles of A, G, C, T, deleted.

What is timed.  wn_phase_links and wn_haplotag through the C ABI on preallocated tables beside wn_pileup_evidence through the C ABI
on the same reads in the same process -- the same walk, which adds three 64-bit cells for EVERY column where the new kernels look a
site up for every column and add only where there is one; wn_phase_chain on the links; and the three functions through the Python
surface with their allocations.  Device events around `reps` calls after `warmup` calls, reps raised until the window is at least
--min-seconds; every window is taken --repeats times and the median is reported with the least and the greatest (tools/gputime.py,
DESIGN.md section 7q's protocol).  Before any time is printed, `observed` must equal the counts of wn_pileup at the sites.  No speed
is asserted.  At this mean depth (1.4) few reads link two sites and almost no two reads share a link cell: the real-coverage case is not measured.
Usage: phase_bench.py [--reads N] [--reference N] [--site-every N] [--reach N] [--reps N] [--warmup N] [--min-seconds S] [--repeats N]
[--out FILE]"""
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
    ap.add_argument("--site-every", type=int, default=500)
    ap.add_argument("--reach", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "phase_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "phase_bench.py measures the GPU; there is no CPU path"
    import wavenet_speech_amd as W
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(47)
    R, max_ins, reach = a.reference, 4, a.reach
    host = make_reads(rng, a.reads, R)
    ops, ops_len, lo, ref_len, strand, query, query_len = (torch.from_numpy(x).to(dev) for x in host)
    qual = torch.from_numpy(rng.integers(0, 41, size=host[5].shape).astype(np.uint8)).to(dev)
    B, width, M = ops.shape[0], ops.shape[1], query.shape[1]
    aln = W.PairwiseAlignment(None, None, None, None, None, ops, ops_len)
    reads = (aln, lo, ref_len, strand, query, query_len)

    # the planted sites
    pos = np.flatnonzero(rng.random(R) < 1.0 / a.site_every).astype(np.int32)
    S = len(pos)
    first = rng.integers(0, 5, size=S)
    pairs = np.sort(np.stack([first, (first + rng.integers(1, 5, size=S)) % 5], 1), 1)           # two different allele indices, ascending
    alleles = ((pairs + 1) % 5).astype(np.uint8)                                                 # as labels: index 4, the deletion, is 0 and last
    site_of = np.full(R, -1, dtype=np.int32)
    site_of[pos] = np.arange(S, dtype=np.int32)
    sites = W.PhaseSites(*(torch.from_numpy(x).to(dev) for x in (pos, alleles, site_of)))

    table = W.genotype_weights().checked("phase_bench")
    counts = torch.zeros(R, 2, 6, dtype=torch.int32, device=dev)
    ins_lengths = torch.zeros(R, max_ins + 1, dtype=torch.int32, device=dev)
    ins_bases = torch.zeros(R, max_ins, 4, dtype=torch.int32, device=dev)
    evidence = torch.zeros(R, 5, 3, dtype=torch.int64, device=dev)
    links = torch.zeros(S, reach, 2, dtype=torch.int64, device=dev)
    observed = torch.zeros(S, 3, dtype=torch.int32, device=dev)
    used = torch.empty(B, dtype=torch.int8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    read_args = lambda q: (_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_len), _p(strand), _p(query), query.stride(0), _p(query_len), _p(q),   # noqa: E731
                           q.stride(0) if q is not None else 0, None, B, M, width, R)
    min_qual = lambda q: 7 if q is not None else 0                   # noqa: E731

    def evidence_kernel(q=None):
        _lib.check(lib.wn_pileup_evidence(*read_args(q), None, ctypes.cast(table, ctypes.c_void_p), 20, 20, min_qual(q), _p(evidence), _p(used),
                                          _p(bad), _stream()), "wn_pileup_evidence")

    def links_kernel(q=None, into=links, seen=observed):
        _lib.check(lib.wn_phase_links(*read_args(q), None, 20, 20, min_qual(q), _p(sites.site_of), _p(sites.alleles), S, reach, _p(into), _p(seen),
                                      _p(used), _p(bad), _stream()), "wn_phase_links")

    # the walks pick the same columns: `observed` is the pileup's count of the two alleles, and of everything else that is no `other`
    _lib.check(lib.wn_pileup(*read_args(qual), 7, max_ins, _p(counts), _p(ins_lengths), _p(ins_bases), _p(used), _p(bad), _stream()), "wn_pileup")
    links_kernel(qual)
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and int((used != 1).sum()) == 0
    at = counts[sites.pos.long()][:, :, :5].sum(1)                   # [S, 5] over both strands, columns A, G, C, T, deletion
    col = (sites.alleles.long() + 4) % 5                             # label k is column k - 1, the deleted allele column 4
    both = torch.gather(at, 1, col)
    assert torch.equal(observed[:, :2].long(), both.long()), "the link walk differs from the pileup's"
    assert torch.equal(observed.long().sum(1), at.long().sum(1)), "the link walk differs from the pileup's"
    del counts, ins_lengths, ins_bases, at

    first_links = W.PhaseLinks(links.clone(), observed.clone(), used.clone())
    phasing = W.phase_chain(first_links, sites)
    chain_out = [torch.empty(S, dtype=t.dtype, device=dev) for t in phasing]
    work = torch.empty(2 * S, dtype=torch.int32, device=dev)
    hp = torch.empty(B, dtype=torch.uint8, device=dev)
    ps = torch.empty(B, dtype=torch.int32, device=dev)
    weight, n_sites = (torch.empty(B, 2, dtype=torch.int32, device=dev) for _ in range(2))

    def chain_kernel():
        parent, flip, margin, root, parity, ps_s, set_size = chain_out
        _lib.check(lib.wn_phase_chain(_p(first_links.links), _p(sites.pos), S, reach, 1, _p(parent), _p(flip), _p(margin), _p(root), _p(parity),
                                      _p(ps_s), _p(set_size), _p(work), _stream()), "wn_phase_chain")

    def tag_kernel(q=None):
        _lib.check(lib.wn_haplotag(*read_args(q), None, 20, 20, min_qual(q), _p(sites.site_of), _p(sites.alleles), S, _p(sites.pos), _p(phasing.root),
                                   _p(phasing.parity), _p(phasing.set_size), _p(hp), _p(ps), _p(weight), _p(n_sites), _p(bad), _stream()),
                   "wn_haplotag")

    tags = W.haplotag(*reads, sites, phasing, qual=qual, min_qual=7)
    columns = int(ops_len.sum())
    rep = Report()
    lines = ["# phase: %d reads of %d..%d op columns (rows of %d; queries of at most %d) on a reference of %d, both strands, quals 0..40, %s"
             % (B, int(ops_len.min()), int(ops_len.max()), width, M, R, torch.cuda.get_device_name(0)),
             "# %d op columns; %d planted sites, %d observations, %d non-zero link cells at reach %d; %d sites in %d sets of more than one; %d of %d reads tagged"
             % (columns, S, int(first_links.observed.sum()), int((first_links.links != 0).sum()), reach, int((phasing.set_size > 1).sum()),
                int(((phasing.set_size > 1) & (phasing.root == torch.arange(S, device=dev))).sum()), int((tags.hp != 0).sum()), B),
             "%-44s %10s %10s %10s %6s" % ("stage", "median ms", "least", "greatest", "reps")]
    for line in lines:
        rep.emit(line)
    times = {}
    for name, fn in (("evidence (wn_pileup_evidence, no qual)", evidence_kernel),
                     ("links (wn_phase_links, no qual)", links_kernel),
                     ("haplotag (wn_haplotag, no qual)", tag_kernel),
                     ("evidence (wn_pileup_evidence, qual)", lambda: evidence_kernel(qual)),
                     ("links (wn_phase_links, qual)", lambda: links_kernel(qual)),
                     ("haplotag (wn_haplotag, qual)", lambda: tag_kernel(qual)),
                     ("chain (wn_phase_chain, %d launches)" % (3 + max(S - 1, 0).bit_length()), chain_kernel),
                     ("phase_links (python, fresh tables)", lambda: W.phase_links(*reads, sites, qual=qual, min_qual=7, reach=reach)),
                     ("phase_chain (python)", lambda: W.phase_chain(first_links, sites)),
                     ("haplotag (python)", lambda: W.haplotag(*reads, sites, phasing, qual=qual, min_qual=7))):
        t = timed(fn, calls=a.reps, windows=a.repeats, warmup=a.warmup, min_seconds=a.min_seconds)
        times[name] = t.median
        rep.emit("%-44s %10.4f %10.4f %10.4f %6d" % (name, t.median, t.least, t.greatest, t.calls))
    rep.emit("links / evidence: %.2fx without qual, %.2fx with; haplotag / evidence: %.2fx, %.2fx; links: %.3g op columns/s; chain: %.3g sites/s" % (
        times["links (wn_phase_links, no qual)"] / times["evidence (wn_pileup_evidence, no qual)"],
        times["links (wn_phase_links, qual)"] / times["evidence (wn_pileup_evidence, qual)"],
        times["haplotag (wn_haplotag, no qual)"] / times["evidence (wn_pileup_evidence, no qual)"],
        times["haplotag (wn_haplotag, qual)"] / times["evidence (wn_pileup_evidence, qual)"],
        columns / (1e-3 * times["links (wn_phase_links, qual)"]),
        S / (1e-3 * [v for k, v in times.items() if k.startswith("chain")][0])))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
