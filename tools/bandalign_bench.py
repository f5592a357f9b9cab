#!/usr/bin/env python3
"""Time banded alignment (csrc/wn_bandalign.hip through wavenet_speech_amd.banded_align) beside the unchanged pairwise_align on the
same pairs: 32 pairs of about 400 labels at width 64, 4096 pairs of about 1200 labels at width 128 and one pair
of 8192 x 8192 at width 256 -- a random reference and a query made from it by 15 % substitutions, insertions and deletions,
needle's costs, free end gaps, the stripe centred on the main diagonal.  Reports ms per batch (median, least, greatest of the
windows) of the full form and of the score-only form of both (the same costs and end-gap rule in all four: the full kernel's
score-only form is called as pairwise_align calls its kernel, without ops and counts), their ratio and both workspaces.  Before
any time is printed, every pair whose full path lies inside its stripe (band_from_ops of pairwise_align's row) is held to equality
of score, counts and ops.
Usage: bandalign_bench.py [--windows N] [--warmup N] [--quick] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet_speech_amd import _lib  # noqa: E402
from wavenet_speech_amd import decoding as D  # noqa: E402

from gputime import Report, timed  # noqa: E402
from pairalign_bench import mutate  # noqa: E402

NEEDLE = (10, -8, 20, 1)                      # needle's costs in half units: the score-only form of the full kernel takes them as they are


def make_pairs(B, n, seed, distinct=64):
    """B pairs as device rows; beyond `distinct` the pairs repeat (the kernels do not know)"""
    rng = np.random.default_rng(seed)
    a = np.zeros((B, n), dtype=np.int32)
    b = np.zeros((B, n), dtype=np.int32)
    an, bn = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for k in range(min(B, distinct)):
        r = rng.integers(1, 5, size=n).tolist()
        q = mutate(rng, r, 0.15)[:n]
        a[k, :len(r)], b[k, :len(q)], an[k], bn[k] = r, q, len(r), len(q)
    for k in range(distinct, B):
        a[k], b[k], an[k], bn[k] = a[k % distinct], b[k % distinct], an[k % distinct], bn[k % distinct]
    return [torch.tensor(v, device="cuda:0") for v in (a, an, b, bn)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="the 32 short pairs only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "bandalign_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bandalign_bench.py measures the GPU; there is no CPU path"
    lib = _lib.load()
    shapes = [(32, 400, 64)] if a.quick else [(32, 400, 64), (4096, 1200, 128), (1, 8192, 256)]
    rep = Report()
    rep.emit("# banded beside full pairwise alignment, needle's costs, free end gaps, int32 labels, %s; median (least .. greatest) of %d "
             "windows, warmup %d" % (torch.cuda.get_device_name(0), a.windows, a.warmup))
    rep.emit("%5s %5s %5s %7s | %-28s %-28s %6s | %-28s %-28s %6s | %9s %9s" % (
        "B", "N", "width", "in band", "banded ms/batch", "full ms/batch", "ratio", "banded score-only", "full score-only", "ratio",
        "banded MB", "full MB"))
    for B, n, width in shapes:
        ref, rl, query, ql = make_pairs(B, n, 1000 * B + n)
        lo = torch.full((B,), -(width // 2), dtype=torch.int32, device="cuda:0")
        hi = lo + (width - 1)
        full = D.pairwise_align(ref, rl, query, ql)
        band = D.banded_align(ref, rl, query, ql, lo, hi, width)
        plo, phi = D.band_from_ops(full)
        inside = (plo >= lo) & (phi <= hi)                           # property 1 applies: the result must be the full one
        for u, v in zip(band.alignment, full):
            assert torch.equal(u[inside], v[inside]), "banded and full alignment differ on a pair whose path is in band"
        assert bool((band.alignment.score <= full.score).all()) and bool((band.edge_hits[inside & (plo > lo) & (phi < hi)] == 0).all())
        only = D.banded_align(ref, rl, query, ql, lo, hi, width, score_only=True)
        assert torch.equal(only.alignment.score, band.alignment.score)
        t = [timed(fn, windows=a.windows, warmup=a.warmup) for fn in (
            lambda: D.banded_align(ref, rl, query, ql, lo, hi, width), lambda: D.pairwise_align(ref, rl, query, ql),
            lambda: D.banded_align(ref, rl, query, ql, lo, hi, width, score_only=True),
            lambda: D._pair_align("pairwise_align", ref, rl, query, ql, NEEDLE, True, False, False))]
        cell = ["%.3f (%.3f .. %.3f)" % (x.median, x.least, x.greatest) for x in t]
        rep.emit("%5d %5d %5d %7d | %-28s %-28s %6.2f | %-28s %-28s %6.2f | %9.1f %9.1f" % (
            B, n, width, int(inside.sum()), cell[0], cell[1], t[1].median / t[0].median, cell[2], cell[3], t[3].median / t[2].median,
            lib.wn_banded_align_workspace_bytes(B, n, n, width) / 2 ** 20, lib.wn_pair_align_workspace_bytes(B, n, n) / 2 ** 20))
    from wavenet_speech_amd import check_device_flags
    check_device_flags()
    if a.out:
        rep.save(a.out)


if __name__ == "__main__":
    main()
