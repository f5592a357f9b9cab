#!/usr/bin/env python3
"""Time the CIGAR encoder and decoder (csrc/wn_cigar.hip: wn_cigar_encode, wn_cigar_decode) on the GPU on op strings drawn as
tools/pileup_bench.py draws them: 4096 reads of 3600..4400 op columns (3 % mismatches, 3 % deletions, 4 % insertions in runs, eight
end columns on either side, both strands), about 4000 bases at about 10 % error.  The decoder is fed the encoder's own run table
and random labels (it is not strict: op 1 / 2 follow the labels, the work is the same).

What is timed.  Each entry point through the C ABI into preallocated outputs (the kernel and its launch, nothing else), beside
wn_pileup through the C ABI on the same strings in the same process: all three walk every column once, so that launch is the
yardstick.  Device events around `reps` calls after `warmup` calls, reps raised until the window is at least --min-seconds; every
window is taken --repeats times and the median is reported with the least and the greatest.  No speed is asserted.
Usage: cigar_bench.py [--reads N] [--reps N] [--warmup N] [--min-seconds S] [--repeats N] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "cigar_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cigar_bench.py measures the GPU; there is no CPU path"
    import wavenet_speech_amd as W
    from wavenet_speech_amd import _lib
    from wavenet_speech_amd._args import _p, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(53)
    R, max_ins = 4600000, 4
    h = make_reads(rng, a.reads, R, lo=3600, hi=4400)
    ops, ops_len, lo, ref_len, strand, query, query_len = (torch.from_numpy(x).to(dev) for x in h)
    reference = torch.from_numpy(rng.integers(1, 5, R).astype(np.int32)).to(dev)
    B, width = ops.shape
    M = int(query.shape[1])
    max_cigar = min(width, 2 * M + 1) + 2
    cigar = torch.empty(B, max_cigar, dtype=torch.int32, device=dev)
    n_cigar, fields = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 5, dtype=torch.int32, device=dev)
    used, used_back, used_pile = (torch.empty(B, dtype=torch.int8, device=dev) for _ in range(3))
    back = torch.empty_like(ops)
    back_len, back_ref, pos = (torch.empty_like(ops_len) for _ in range(3))
    stats = torch.empty(B, 4, dtype=torch.int32, device=dev)
    ws_bytes = lib.wn_cigar_decode_workspace_bytes(B, max_cigar)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.zeros(R, 2, 6, dtype=torch.int32, device=dev)
    ins_lengths = torch.zeros(R, max_ins + 1, dtype=torch.int32, device=dev)
    ins_bases = torch.zeros(R, max_ins, 4, dtype=torch.int32, device=dev)

    def encode():
        _lib.check(lib.wn_cigar_encode(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_len), _p(strand), _p(query_len), None, B, M, width, R, 1,
                                       max_cigar, _p(cigar), cigar.stride(0), _p(n_cigar), _p(fields), _p(used), _p(bad), _stream()), "wn_cigar_encode")

    def decode():
        _lib.check(lib.wn_cigar_decode(_p(cigar), cigar.stride(0), _p(n_cigar), _p(pos), _p(strand), _p(reference), R, _p(query), query.stride(0),
                                       _p(query_len), B, max_cigar, M, width, 0, _p(back), back.stride(0), _p(back_len), _p(back_ref), _p(stats),
                                       _p(used_back), _p(ws), ws_bytes, _p(bad), _stream()), "wn_cigar_decode")

    def pileup_kernel():
        _lib.check(lib.wn_pileup(_p(ops), ops.stride(0), _p(ops_len), _p(lo), _p(ref_len), _p(strand), _p(query), query.stride(0), _p(query_len),
                                 None, 0, None, B, M, width, R, 0, max_ins, _p(counts), _p(ins_lengths), _p(ins_bases), _p(used_pile), _p(bad),
                                 _stream()), "wn_pileup")

    encode()
    pos.copy_(fields[:, 0])                                          # the decoder takes pos [B]: the first column of the fields
    decode()
    pileup_kernel()
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and int((used != 1).sum()) == 0 and int((used_back != 1).sum()) == 0 and int((used_pile != 1).sum()) == 0
    assert torch.equal(back_ref, fields[:, 1]) and torch.equal(((back != 3) & (back != 0)).sum(1).int(), query_len)      # the spans and the labels consumed
    rows = W.cigar_runs(W.PairwiseAlignment(None, None, None, None, None, ops, ops_len), lo, ref_len, strand, query_len, R, max_cigar=max_cigar)
    assert torch.equal(rows.cigar, cigar) and torch.equal(rows.n_cigar, n_cigar)
    rep = Report()
    for line in ("# cigar: %d reads of %d..%d op columns (rows of %d), at most %d labels, both strands, = / X runs, %s"
                 % (B, int(ops_len.min()), int(ops_len.max()), width, M, torch.cuda.get_device_name(0)),
                 "# %d op columns, %d runs (%.1f columns per run, at most %d of %d per row), workspace %d bytes"
                 % (int(ops_len.sum()), int(n_cigar.sum()), float(ops_len.sum()) / float(n_cigar.sum()), int(n_cigar.max()), max_cigar, ws_bytes),
                 "%-34s %10s %10s %10s %6s" % ("stage", "median ms", "least", "greatest", "reps")):
        rep.emit(line)
    times = {}
    for name, fn in (("encode (wn_cigar_encode)", encode), ("decode (wn_cigar_decode)", decode), ("pileup (wn_pileup)", pileup_kernel)):
        t = timed(fn, calls=a.reps, windows=a.repeats, warmup=a.warmup, min_seconds=a.min_seconds)
        times[name] = t.median
        rep.emit("%-34s %10.4f %10.4f %10.4f %6d" % (name, t.median, t.least, t.greatest, t.calls))
    for name in ("encode (wn_cigar_encode)", "decode (wn_cigar_decode)"):
        rep.emit("%s: %.3g op columns/s, %.2fx the time of wn_pileup on the same strings" % (
            name.split()[0], int(ops_len.sum()) / (times[name] * 1e-3), times[name] / times["pileup (wn_pileup)"]))
    W.check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
