"""The cases the CPU and GPU tests of banded alignment share (tests/test_banded_align_ref.py, tests/test_gpu_banded_align.py):
cost sets, pair generators and the widths at which csrc/wn_bandalign.hip changes hands."""
import numpy as np

from tests.pairwise_align_ref import EMBOSS, UNIT

# every set has gap_open > 0, so a path never ends or begins with a gap that costs nothing more than the end gap beside it: the
# path cells read off an op row (banded_align_ref.path_cells) are then exactly the cells the trace visited
COSTS = (EMBOSS, UNIT, (2, -3, 5, 2), (1, -1, 2, 0), (3, -2, 4, 4))

PER = 8                                  # diagonals per thread (kBaPer)
WAVE = 64 * PER                          # the widest stripe of the one-wave form
MAX_BAND = 2048
# every ownership edge: threads, the wave, the waves of the 256-thread form, the limit
WIDTHS = (1, 2, 3, PER - 1, PER, PER + 1, WAVE - 1, WAVE, WAVE + 1, 1023, 1024, 1025, 2047, 2048)
# label rings (kRing / kFill): the one-wave form refills 512 labels into 1024, the 256-thread form 1024 into 4096; the trace
# walks windows of 64 lookups (kBaChunk)
FILL_ONE_WAVE, FILL_MULTI, TRACE_CHUNK = 512, 1024, 64


def mutate(rng, a, rate, letters):
    """a with `rate` of its labels substituted, deleted or followed by an insertion"""
    out = []
    for v in a:
        r = rng.random()
        if r < rate / 3:
            continue
        out.append(int(rng.integers(1, letters + 1)) if r < 2 * rate / 3 else int(v))
        if r > 1 - rate / 3:
            out.append(int(rng.integers(1, letters + 1)))
    return np.array(out, dtype=np.int64)


def random_pair(rng, n, m, letters, related):
    a = rng.integers(1, letters + 1, size=n)
    if not related:
        return a, rng.integers(1, letters + 1, size=m)
    b = mutate(rng, a, 0.15, letters)
    if len(b) < m:
        b = np.concatenate([b, rng.integers(1, letters + 1, size=m - len(b))])
    return a, b[:m]


def random_stripe(rng, n, m, max_width):
    """a stripe that meets the rectangle, at most max_width wide, somewhere about the main path"""
    centre = int(rng.integers(min(-2, m - n - 3), max(2, m - n + 3) + 1))
    width = int(rng.integers(1, max_width + 1))
    lo = centre - width // 2
    lo = min(max(lo, -n - width + 1), m)
    return lo, lo + width - 1


# ---- realign(first=, band=) on the planted phased runs of tests/realign_cases.py, from the host run (the quadratic host aligner for the
# full form, tests/banded_align_ref.py inside [lo1 - n4 - band, hi1 + n3 + band] for the banded one), by `noisy`
REALIGN_BAND = 16                             # no pick differs at 16, so no wider margin is needed
REALIGN_DIFFER = {False: 0, True: 0}          # reads whose pick, hp or lifted row differs from the full run's, of 160
REALIGN_LOWER = {False: 0, True: 0}           # (read, haplotype) scores below the full run's, of 320; none is above
REALIGN_WIDEST = 47                           # diagonals of the widest stripe
