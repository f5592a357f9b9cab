#!/usr/bin/env python3
"""Time the signal-to-reference mapping (csrc/wn_sigmap.hip: wn_signal_map, two launches) on the GPU.

A random 48 502-base reference (the length of lambda) on both strands, B in {1, 32, 256} reads, their first T in {512, 2048, 4096}
samples, strip automatic and two hand values; and one 4.6 M-base reference (both strands) with B = 4, T = 2048.  Reads are cut from
either strand at random and generated on the device by ragged_reads (gamma dwell of about 8 samples per k-mer, the "generator"
window, the stand-in table).  Device events around the C ABI call alone (buffers allocated beforehand); after one warm-up call the
number of timed calls is chosen so that a shape takes about two seconds (between 2 and 20); min / median / max ms.  Gcell/s counts
the cells of the definition, M * sum T_b, at the median: the halo columns a workgroup computes and throws away are not counted, and
their share of all computed columns (whole tiles, from the strip rule of DESIGN.md section 7l, mirrored in halo_share below) is
printed beside it.  "found" is the share of reads whose start lies within 2 states of the stretch they were cut from.

Writes its table to --out, by default profiles/rNN/signal_map_bench.txt in the next free rNN.
Usage: signal_map_bench.py [--out FILE] [--quick] [--seconds S]"""
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

DWELL = ("gamma", 4.0, 2000.0, 4000.0)          # mean 8 samples, shape 4
TILE, FULL_CHIP = 1024, 512                     # csrc/wn_sigmap.hip: kSmTile, kSmFullChip


def up64(v):
    return (v + 63) // 64 * 64


def auto_strip(B, L, M):
    """the library's choice (csrc/wn_sigmap.hip: sm_auto_strip)"""
    strip, floor = up64(8 * L), up64(L)
    while strip // 2 >= floor and B * ((M + strip - 1) // strip) < FULL_CHIP:
        strip = up64(strip // 2)
    return min(strip, 1 << 20)


def halo_share(lengths, M, strip):
    """the share of computed columns (whole tiles) that no workgroup owns, over the reads of a batch"""
    computed = 0
    for T in lengths:
        for own0 in range(0, M, strip):
            first = max(own0 - up64(T - 1), 0)
            computed += -(-(min(own0 + strip, M) - first) // TILE) * TILE
    return 1.0 - M * len(lengths) / computed


def make_reads(reference, B, T, seed, dev):
    """B reads cut from the joined reference (either strand), enough bases for T samples; (signal [B, T], lengths, true start)"""
    g = torch.Generator().manual_seed(seed)
    n = max(T // 4, 16)                                              # about 2 T samples at a mean dwell of 8
    half = reference.R
    strand = torch.randint(0, 2, (B,), generator=g)
    pos = torch.randint(0, half - n + 1, (B,), generator=g)
    start = (pos + strand * (half + 1)).to(dev)
    bases = reference.bases[start[:, None] + torch.arange(n, device=dev)[None, :]]
    reads = S.ragged_reads(B, dwell=DWELL, window="generator", bases=bases, generator=g, device=dev, pad_to=16 * n)
    signal = reads.signal[:, 0, :T].contiguous()
    return signal, reads.signal_lengths.clamp(max=T).int().contiguous(), start


def time_shape(lib, reference, B, T, strip, seconds, dev):
    signal, lengths, truth = make_reads(reference, B, T, 100 + B + T, dev)
    model, M, k = reference.model, reference.n_states, reference.k
    G = (M + 63) // 64
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    score, runner, block_cost = torch.empty(B, **i64), torch.empty(B, **i64), torch.empty(B, G, **i64)
    end, start, block_end, bad = torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(B, G, **i32), torch.zeros(1, **i32)
    ws_bytes = lib.wn_signal_map_workspace_bytes(B, T, reference.ref_len, k, strip)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def abi():
        _lib.check(lib.wn_signal_map(_p(signal), 0, signal.stride(0), _p(lengths), None, _p(reference.prepared), reference.ref_len, k, B, T,
                                     model.frac_bits, model.weight_shift, 2 ** 31 - 1, strip, _p(score), _p(end), _p(start), _p(runner),
                                     _p(block_cost), _p(block_end), None, _p(ws), ws_bytes, _p(bad), _stream()), "wn_signal_map")

    warm = timed(abi).median                                         # the warm-up call
    reps = max(2, min(20, int(seconds * 1e3 / max(warm, 1e-3))))
    times = timed(abi, windows=reps).ms
    assert int(bad) == 0
    cells = M * int(lengths.sum())
    used = strip or auto_strip(B, T, M)
    found = float(((start.long() - truth).abs() <= 2).double().mean())
    ahead = float((runner.double() / score.double()).median())
    return "%5d %6d %9d %8s %4d %30s %10.2f %7.3f %7.3f %9.3f" % (B, T, M, "auto %d" % used if not strip else "%d" % strip, reps,
                                                               "%.3f / %.3f / %.3f" % (times[0], times[len(times) // 2], times[-1]),
                                                               cells / (times[len(times) // 2] * 1e-3) / 1e9,
                                                               halo_share(lengths.tolist(), M, used), found, ahead)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=2.0, help="the time a shape's timed calls should take together")
    ap.add_argument("--quick", action="store_true", help="B = 32 on the short reference only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "signal_map_bench.py measures the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    model = W.signal_model(*S.standin_kmer_table())
    g = torch.Generator().manual_seed(7)
    rep = Report()
    lines = ["# signal_map: k=%d, frac_bits=%d, weight_shift=%d, dwell %s, both strands, %s; device events around wn_signal_map (both "
             "launches); one warm-up call, then `n` timed calls (about %.1f s per shape); ms per call: min / median / max; Gcell/s = M * "
             "sum T_b / median, halo excluded" % (model.k, model.frac_bits, model.weight_shift, DWELL, torch.cuda.get_device_name(0), a.seconds),
             "%5s %6s %9s %8s %4s %30s %10s %7s %7s %9s" % ("reads", "T", "states", "strip", "n", "ms", "Gcell/s", "halo", "found", "2nd/best")]
    for line in lines:
        rep.emit(line)
    small = W.map_reference(torch.randint(1, 5, (48502,), generator=g), model, device=dev)
    shapes = [(small, B, T, strip) for B in ((32,) if a.quick else (1, 32, 256)) for T in (512, 2048, 4096) for strip in (0, 2048, 16384)]
    if not a.quick:
        shapes.append((W.map_reference(torch.randint(1, 5, (4600000,), generator=g), model, device=dev), 4, 2048, 0))
    for reference, B, T, strip in shapes:
        line = time_shape(lib, reference, B, T, strip, a.seconds, dev)
        rep.emit(line)
    W.check_device_flags()
    out = a.out or os.path.join(next_profile_dir(), "signal_map_bench.txt")
    rep.save(out)
    print("wrote", out)


if __name__ == "__main__":
    main()
