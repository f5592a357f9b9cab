"""The inputs of the demultiplexing tests (tests/test_gpu_demux.py on the device, tests/test_demux_ref.py on the CPU) and their
references by tests/demux_ref.py, built once per process.  Costs here are the doubled integers the kernel works in (the Python
surface takes them halved).  The shapes are the smallest at which the kernel takes another path: the wave edge of 64 patterns per
end, the row-bound templates of 32, 64, 96 and 128 rows, the group of 8 rows after which a wave leaves the
row loop, windows shorter than the pattern, reads shorter than the window."""
import functools
from collections import namedtuple

import numpy as np

from tests import demux_ref as R

Case = namedtuple("Case", "labels lengths patterns pattern_lengths n_front group window costs")
PORECHOP = (6, -12, 10, 4)               # match 3, mismatch -6, gap open 5, gap extend 2, doubled


def _rows(seqs, width=None):
    width = max([len(s) for s in seqs] + [1]) if width is None else width
    out = np.zeros((len(seqs), width), dtype=np.int32)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, np.array([len(s) for s in seqs], dtype=np.int32)


def _case(reads, front, rear, window, costs=PORECHOP, group=None, width=None):
    labels, lengths = _rows(reads, width)
    patterns, plen = _rows(list(front) + list(rear))
    group = list(range(len(front))) + list(range(len(rear))) if group is None else group
    return Case(labels, lengths, patterns, plen, len(front), np.array(group, dtype=np.int32), window, costs)


def _rand(rng, n, labels=4):
    return [int(v) for v in rng.integers(1, labels + 1, n)]


def _mixed(rng, count, lo, hi):
    return [_rand(rng, int(rng.integers(lo, hi + 1))) for _ in range(count)]


def _build():
    c = {}
    # worked by hand (tests/test_demux_ref.py): costs 2, -2, 3, 1
    c["hand"] = _case([[4, 1, 2, 3, 4]], [[1, 2, 3]], [[2, 3, 1]], 5, (2, -2, 3, 1))
    rng = np.random.default_rng(20261019)
    reads = [_rand(rng, n) for n in (30, 17, 0, 1, 64)]              # a read of length 0 among the others
    c["p1"] = _case(reads, [[1], [2], [3]], [[4], [1]], 8)
    c["window1"] = _case(reads, _mixed(rng, 3, 1, 6), _mixed(rng, 3, 1, 6), 1)
    c["longer_than_window"] = _case(reads, _mixed(rng, 3, 9, 12), _mixed(rng, 3, 9, 12), 4)
    c["short_reads"] = _case([_rand(rng, n) for n in (7, 3, 9, 10, 11)], _mixed(rng, 4, 3, 6), _mixed(rng, 4, 3, 6), 10)
    # the wave edge: 1, 63, 64 and 65 patterns per end, lengths mixed in one wave (the latch row; 1..12 also crosses the row group)
    two = [_rand(rng, 40), _rand(rng, 11)]
    c["k_1_64"] = _case(two, _mixed(rng, 1, 1, 12), _mixed(rng, 64, 1, 12), 16)
    c["k_63_65"] = _case(two, _mixed(rng, 63, 1, 12), _mixed(rng, 65, 1, 12), 16)
    c["k_64_63"] = _case(two, _mixed(rng, 64, 1, 12), _mixed(rng, 63, 1, 12), 16)
    c["front_only"] = _case(two, _mixed(rng, 65, 1, 12), [], 16)
    c["rear_only"] = _case(two, [], _mixed(rng, 3, 1, 12), 16)
    # the row-bound templates: the longest pattern at 32 | 33, 64 | 65 and 96 | 97, shorter ones beside it
    for pmax in (8, 9, 32, 33, 64, 65, 96, 97):
        lens = (pmax, 1, max(1, pmax - 1), max(1, pmax // 2))
        c["rows_%d" % pmax] = _case([_rand(rng, 50), _rand(rng, 20)], [_rand(rng, n) for n in lens], [_rand(rng, n) for n in lens[::-1]], 24)
    big = [_rand(rng, 600)]
    c["p128_w512"] = _case(big, [_rand(rng, 128), _rand(rng, 5)], [_rand(rng, 128)], 512)
    # ties: a homopolymer read and pattern (every start ties: the smallest start and end), and two labels only
    c["homopolymer"] = _case([[1] * 30, [1] * 4], [[1] * 5, [1]], [[1] * 5, [1] * 6], 20)
    c["two_labels"] = _case([_rand(rng, 40, 2), _rand(rng, 9, 2)], [_rand(rng, n, 2) for n in (6, 3, 10)], [_rand(rng, n, 2) for n in (6, 2)], 12)
    # the costs: both limits at the largest shape (score range, the sentinel), ge = 0, go = ge, a reward for a mismatch
    c["costs_limit"] = _case(big, [big[0][100:228]], [_rand(rng, 128)], 512, (1024, -1024, 1024, 1024))
    small = [_rand(rng, 40, 3), _rand(rng, 10, 3)]
    pats = [_rand(rng, n, 3) for n in (7, 12, 3)]
    c["ge_0"] = _case(small, pats, pats, 16, (6, -12, 10, 0))
    c["go_eq_ge"] = _case(small, pats, pats, 16, (6, -12, 4, 4))
    c["all_zero_gaps"] = _case(small, pats, pats, 16, (2, -2, 0, 0))
    c["negative_match"] = _case(small, pats, pats, 16, (-1024, 1024, 1024, 0))
    return c


CASES = _build()


@functools.lru_cache(maxsize=None)
def reference(name):
    case = CASES[name]
    return R.demux_scores_ref(case.labels, case.lengths, case.patterns, case.pattern_lengths, case.n_front, case.window, *case.costs)


# ---- the planted run: 64 reads of 200-400 random bases, one of 12 barcodes of 24 bases at the front and its reverse complement at
# the rear, both corrupted by substitutions, insertions and deletions at a fixed rate; some reads miss one end
PLANT_READS, PLANT_CODES, PLANT_LEN, PLANT_WINDOW, PLANT_ERROR = 64, 12, 24, 40, 0.08
PLANT_MIN_DISTANCE = 12                  # pairwise edit distance of the barcode set, reverse complements included
PLANT_FRACTION, PLANT_MARGIN = 0.6, 6.0
COMPLEMENT = (0, 4, 3, 2, 1)


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def revcomp(seq):
    return [COMPLEMENT[v] for v in reversed(seq)]


def _corrupt(rng, seq, rate):
    out = []
    for v in seq:
        u = rng.random()
        if u < rate / 3:
            continue                                                 # deletion
        if u < 2 * rate / 3:
            out.append(int(rng.integers(1, 5)))                      # insertion before it
        elif u < rate:
            v = int((v - 1 + rng.integers(1, 4)) % 4 + 1)            # substitution by another base
        out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def planted():
    """dict: codes (the 12 barcodes), case (the Case: front patterns = the barcodes, rear = their reverse complements, group =
    barcode), truth [64] (the planted barcode), has_front / has_rear [64], seqs (the reads as lists)"""
    rng = np.random.default_rng(7)
    codes = []
    while len(codes) < PLANT_CODES:                                  # greedy: far from every barcode and reverse complement so far
        cand = _rand(rng, PLANT_LEN)
        if all(edit_distance(cand, o) >= PLANT_MIN_DISTANCE for c in codes for o in (c, revcomp(c))) \
                and edit_distance(cand, revcomp(cand)) >= PLANT_MIN_DISTANCE:
            codes.append(cand)
    truth = rng.integers(0, PLANT_CODES, PLANT_READS)
    has_front = np.ones(PLANT_READS, dtype=bool)
    has_rear = np.ones(PLANT_READS, dtype=bool)
    has_front[[5, 21, 40]] = False
    has_rear[[9, 33, 50, 63]] = False
    seqs = []
    for b in range(PLANT_READS):
        body = _rand(rng, int(rng.integers(200, 401)))
        head = _rand(rng, int(rng.integers(0, 7))) + _corrupt(rng, codes[truth[b]], PLANT_ERROR) if has_front[b] else []
        tail = _corrupt(rng, revcomp(codes[truth[b]]), PLANT_ERROR) + _rand(rng, int(rng.integers(0, 7))) if has_rear[b] else []
        seqs.append(head + body + tail)
    case = _case(seqs, codes, [revcomp(c) for c in codes], PLANT_WINDOW)
    return dict(codes=codes, case=case, truth=truth.astype(np.int32), has_front=has_front, has_rear=has_rear, seqs=seqs)


def min_scores(case, fraction_num, fraction_den):
    """ceil(fraction * match * P_k) per pattern, match being the doubled integer: exact integer arithmetic"""
    m = case.costs[0]
    return np.array([-((-fraction_num * m * int(P)) // fraction_den) for P in case.pattern_lengths], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def planted_reference():
    """(scores, pick) of the planted run by the reference, with min_fraction 0.6 and min_margin 6 (12 in half units)"""
    case = planted()["case"]
    s = R.demux_scores_ref(case.labels, case.lengths, case.patterns, case.pattern_lengths, case.n_front, case.window, *case.costs)
    pick = R.demux_pick_ref(s["score"], s["start"], s["end"], case.lengths, case.group, min_scores(case, 3, 5), case.n_front,
                            int(2 * PLANT_MARGIN), False)
    return s, pick
