"""GPU: banded global pairwise alignment (csrc/wn_bandalign.hip through wavenet_speech_amd.banded_align and band_from_ops) against
the numpy int64 reference of tests/banded_align_ref.py and against pairwise_align on the same device.

The arithmetic is integer and the tie rule is part of the contract, so EVERYTHING is compared for exact equality: status, score,
the four counts, ops_len, every op and edge_hits.  Next to that, checks that do not depend on any reference: the ops spell both
rows exactly once, rescore to the score, the counts are the op counts and the path cells are in band."""
import json
import os

import numpy as np
import pytest
import torch

from tests import banded_align_ref as R
from tests import pairwise_align_ref as P
from tests.banded_align_cases import COSTS, FILL_MULTI, FILL_ONE_WAVE, PER, TRACE_CHUNK, WAVE, WIDTHS, random_pair, random_stripe
from tests.gpu_calls import capture
from tests.gpu_labels import package as _W, pad_rows as _pad, pair_align as _full
from tests.gpu_util import DEV, assert_equal_arrays, strided
from tests.gpu_util import no_stale_flags  # noqa: F401

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emboss_pairs.json")
BASES = {"A": 1, "G": 2, "C": 3, "T": 4}
INT_MIN = -2 ** 31


def _kw(costs, free):
    return dict(match=costs[0] / 2, mismatch=costs[1] / 2, gap_open=costs[2] / 2, gap_extend=costs[3] / 2, end_gaps_free=free)


def _host(out):
    """a BandedAlignment as host arrays: status, score in half units, stats [B][4] or None, ops, ops_len, edge_hits"""
    torch.cuda.synchronize()
    al = out.alignment
    assert al.score.dtype == torch.float32 and out.status.dtype == torch.int8 and out.status.is_cuda, (al.score.dtype, out.status.dtype)
    score2 = (al.score.double() * 2).cpu().numpy()
    assert (score2 == np.round(score2)).all(), "a score that is no half unit"
    stats = None if al.matches is None else torch.stack([al.matches, al.mismatches, al.gaps, al.length], dim=1).cpu().numpy()
    return (out.status.cpu().numpy(), score2.astype(np.int64), stats, None if al.ops is None else al.ops.cpu().numpy(),
            None if al.ops_len is None else al.ops_len.cpu().numpy(), None if out.edge_hits is None else out.edge_hits.cpu().numpy())


def _banded(refs, queries, stripes, costs, free, max_band=None, ref_width=None, query_width=None, fill=0, **kw):
    a, an = _pad(refs, ref_width, fill)
    b, bn = _pad(queries, query_width, fill)
    lo = torch.tensor([s[0] for s in stripes], dtype=torch.int32, device=DEV)
    hi = torch.tensor([s[1] for s in stripes], dtype=torch.int32, device=DEV)
    if max_band is None:
        max_band = max(s[1] - s[0] + 1 for s in stripes)
    return _host(_W().banded_align(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV), lo, hi, max_band, **_kw(costs, free), **kw))


def _check(refs, queries, stripes, costs, free, got, tag=""):
    """every pair of a device result: equal to the reference in every number, and consistent in itself"""
    status, score, stats, ops, ops_len, hits = got
    wants = []
    for n, (a, b, (lo, hi)) in enumerate(zip(refs, queries, stripes)):
        t = "%s[%d] N %d M %d stripe [%d, %d]" % (tag, n, len(a), len(b), lo, hi)
        want = R.align(a, b, lo, hi, *costs, free)
        wants.append(want)
        assert status[n] == want.status, (t, status[n], want.status)
        assert score[n] == (want.score if want.status else INT_MIN), (t, score[n], want.score)
        if stats is not None:
            assert tuple(stats[n]) == tuple(want[2:6]), (t, tuple(stats[n]), want[2:6])
            assert hits[n] == want.edge_hits, (t, hits[n], want.edge_hits)
        if ops is None:
            continue
        assert ops_len[n] == want.length, (t, ops_len[n], want.length)
        row = ops[n, :ops_len[n]]
        assert_equal_arrays(row, want.ops, t + " ops")
        assert (ops[n, ops_len[n]:] == 0).all(), t + ": ops past ops_len"
        if not want.status:
            continue
        # without the reference
        ra, rb = P.replay(a, b, row)
        assert ra == [int(v) for v in a] and rb == [int(v) for v in b], t + ": the ops do not spell the two rows"
        assert P.rescore(row, *costs, free) == score[n], (t, P.rescore(row, *costs, free), score[n])
        assert (int((row == 1).sum()), int((row == 2).sum()), int((row >= 3).sum()), len(row)) == tuple(stats[n]), (t, tuple(stats[n]))
        if not (free and len(a) * len(b) == 0):                     # a row of end gaps does not say which border cell it was
            cells = R.path_cells(row, free)
            assert all(R.in_band(i, j, lo, hi) for i, j in cells), t + ": a path cell out of band"
            assert hits[n] == sum(j - i in (lo, hi) for i, j in cells), (t, hits[n])
    return wants


def _golden_pairs():
    pairs = json.load(open(GOLDEN))["pairs"]
    return [[BASES[c] for c in p["true"]] for p in pairs], [[BASES[c] for c in p["pred"]] for p in pairs]


def _stripes_of(ops, ops_len, free, margin=0):
    return [R.band_from_ops(ops[n, :ops_len[n]], margin=margin, free=free) for n in range(len(ops_len))]


# ------------------------------------------------------------------------------------------------------- 1. the notebook's pairs

def test_the_notebook_pairs_under_their_own_stripe_and_a_narrower_one():
    refs, queries = _golden_pairs()
    full = _full(refs, queries, P.EMBOSS, True)
    a, an = _pad(refs)
    b, bn = _pad(queries)
    W = _W()
    al = W.pairwise_align(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV))
    lo, hi = W.band_from_ops(al, 0)
    stripes = _stripes_of(full[2], full[3], True)
    assert lo.dtype == torch.int32 and lo.is_cuda and lo.tolist() == [s[0] for s in stripes] and hi.tolist() == [s[1] for s in stripes]
    got = _host(W.banded_align(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV), lo, hi, max(s[1] - s[0] + 1 for s in stripes)))
    assert (got[0] == 1).all()
    for u, v, what in zip(got[1:5], full, ("score", "stats", "ops", "ops_len")):
        assert_equal_arrays(u, v, "notebook " + what)
    _check(refs, queries, stripes, P.EMBOSS, True, got, "notebook")
    wide = _banded(refs, queries, [(s[0] - 1, s[1] + 1) for s in stripes], P.EMBOSS, True)
    assert_equal_arrays(wide[3], full[2], "notebook ops, one diagonal more")
    assert not wide[5].any(), wide[5]
    # three diagonals narrower (where the path has them): the banded reference decides
    narrow = [(s[0], max(s[0], s[1] - 3)) for s in stripes]
    wants = _check(refs, queries, narrow, P.EMBOSS, True, _banded(refs, queries, narrow, P.EMBOSS, True), "notebook narrow")
    assert all(w.score <= f for w, f in zip(wants, full[0]))
    # band_from_ops' margin and clamp on the device
    lo, hi = W.band_from_ops(al, 5, max_band=8)
    want = [R.band_from_ops(full[2][n, :full[3][n]], margin=5, max_band=8) for n in range(len(refs))]
    assert lo.tolist() == [s[0] for s in want] and hi.tolist() == [s[1] for s in want]


# -------------------------------------------------------------------------------------- 2. random pairs, every mode and cost set

@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("costs", [0, 1, 3])
@pytest.mark.parametrize("kind", ["mutated4", "unrelated4", "mutated2", "unrelated2"])
def test_random_pairs_under_random_stripes(kind, costs, free):
    rng = np.random.default_rng(100 + 10 * costs + len(kind) + free)
    letters, related = int(kind[-1]), kind.startswith("mutated")
    refs, queries, stripes = [], [], []
    for n in range(24):
        N, M = int(rng.integers(0, 140)), int(rng.integers(0, 140))
        a, b = random_pair(rng, N, M, letters, related)
        refs.append(a); queries.append(b)
        stripes.append(random_stripe(rng, N, M, 40))
    got = _banded(refs, queries, stripes, COSTS[costs], free, max_band=40)
    _check(refs, queries, stripes, COSTS[costs], free, got, kind)
    # the stripe of the full path gives the full result, and band_from_ops on the device finds it
    full = _full(refs, queries, COSTS[costs], free)
    own = _stripes_of(full[2], full[3], free)
    again = _banded(refs, queries, own, COSTS[costs], free)
    for u, v, what in zip(again[1:5], full, ("score", "stats", "ops", "ops_len")):
        assert_equal_arrays(u, v, "%s under its own stripe: %s" % (kind, what))
    W = _W()
    al = W.PairwiseAlignment(None, None, None, None, None, torch.from_numpy(full[2]).to(DEV), torch.from_numpy(full[3]).to(DEV))
    lo, hi = W.band_from_ops(al, end_gaps_free=free)
    assert lo.tolist() == [s[0] for s in own] and hi.tolist() == [s[1] for s in own]


# ------------------------------------------------------------------------------------------------------ 3. every ownership edge

@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("width", WIDTHS)
def test_widths_at_every_ownership_edge(width, odd):
    """1, 2, 3, G - 1, G, G + 1 diagonals (G = 8 per thread), 64 G -+ 1 (the one-wave form's last width and the first of the 256
    threads), the wave edges inside those, and the limit; N + M even and odd"""
    rng = np.random.default_rng(width + odd)
    N = min(width // 2 + 24, 1500)
    M = N + odd
    a, b = random_pair(rng, N, M, 4, True)
    lo = -(width // 2)
    stripes = [(lo, lo + width - 1), (lo + 3, lo + width + 2)]
    for free in (True, False):
        got = _banded([a, a], [b, b], stripes, P.EMBOSS, free)
        _check([a, a], [b, b], stripes, P.EMBOSS, free, got, "width %d" % width)


@pytest.mark.parametrize("seam", [WAVE, 2 * WAVE, 3 * WAVE])
def test_the_path_runs_along_a_seam_between_two_waves(seam):
    """the stripe is laid so that the main diagonal is the first diagonal of wave seam / 512: the path of a mutated pair crosses the
    seam with every indel, so what lane 63 and lane 0 hand to each other decides the result (a wide stripe about the main diagonal
    keeps its wave seams in corners where no path goes)"""
    rng = np.random.default_rng(seam)
    refs, queries, stripes = [], [], []
    for shift in (0, 1, -1, 2):
        a, b = random_pair(rng, seam + 40 + shift, seam + 41, 4, True)           # N >= seam: the stripe's first diagonal meets the rectangle
        refs.append(a); queries.append(b); stripes.append((-seam + shift, -seam + shift + seam + 100))
    for free in (True, False):
        got = _banded(refs, queries, stripes, P.EMBOSS, free)
        wants = _check(refs, queries, stripes, P.EMBOSS, free, got, "seam %d" % seam)
        assert all(w.gaps > 10 for w in wants)


# ------------------------------------------------------------------------------------------------ 4. where the stripe lies

@pytest.mark.parametrize("free", [True, False])
def test_stripes_over_the_rectangle_at_its_corners_and_width_one(free):
    rng = np.random.default_rng(5)
    N, M = 37, 29
    a, b = random_pair(rng, N, M, 4, True)
    stripes = [(-N - 50, M + 60), (-N - 50, 0), (0, M + 60),         # hanging over the rectangle
               (M, M), (M - 1, M + 9), (-N, -N), (-N - 9, -N + 1),   # touching a corner only
               (M - N, M - N), (0, 0), (3, 3), (-4, -4), (M - N - 1, M - N - 1),      # width 1 on and off the main diagonal
               (M + 1, M + 5), (-N - 5, -N - 1), (M, M + 5), (-N - 5, -N),            # both no-alignment rules (free), each side
               (M - N + 1, M), (-N, M - N - 1), (M - N, M), (-N, M - N)]              # (penalised), each side
    got = _banded([a] * len(stripes), [b] * len(stripes), stripes, P.EMBOSS, free)
    wants = _check([a] * len(stripes), [b] * len(stripes), stripes, P.EMBOSS, free, got, "stripes")
    none = [w.status == 0 for w in wants]
    assert none[12] and none[13] and (none[16] and none[17] if not free else not (none[14] or none[15])), none
    for n in np.nonzero(none)[0]:                                    # no alignment is not a bad pair
        assert got[1][n] == INT_MIN and not got[2][n].any() and got[4][n] == 0 and got[5][n] == 0 and not got[3][n].any()
    _W().check_device_flags()


@pytest.mark.parametrize("free", [True, False])
def test_zero_lengths(free):
    refs = [[], [1, 2, 3], [], [2] * 9, []]
    queries = [[], [], [4, 3, 2, 1], [], [1] * 7]
    stripes = [(0, 0), (-3, 0), (0, 4), (-5, -2), (2, 3)]
    got = _banded(refs, queries, stripes, P.EMBOSS, free)
    _check(refs, queries, stripes, P.EMBOSS, free, got, "zero lengths")


# ------------------------------------------------------------------------------------- 5. label-ring and trace-chunk seams, long pairs

@pytest.mark.parametrize("width,fill", [(24, FILL_ONE_WAVE), (WAVE + 88, FILL_MULTI)])
def test_label_ring_seams(width, fill):
    """the one-wave form refills 512 labels of either row into rings of 1024, the 256-thread form 1024 into 4096: lengths at the
    first and second refill, one less and one more, on the reference and on the query side"""
    rng = np.random.default_rng(fill)
    refs, queries, stripes = [], [], []
    for k in (1, 2):
        for e in (-1, 0, 1):
            for N, M in ((fill * k + e, fill * k + 7), (fill * k - 9, fill * k + e)):
                a, b = random_pair(rng, N, M, 4, True)
                refs.append(a); queries.append(b)
                stripes.append((M - N - width // 2, M - N - width // 2 + width - 1))
    got = _banded(refs, queries, stripes, P.EMBOSS, True)
    _check(refs, queries, stripes, P.EMBOSS, True, got, "ring seams")


def test_trace_chunk_seams():
    """the trace walks windows of 64 lookups: paths of 64 k - 1, 64 k and 64 k + 1 diagonal moves, and paths with long gaps that cross
    a window's diagonal range"""
    rng = np.random.default_rng(64)
    refs, queries, stripes = [], [], []
    for k in (1, 2, 3):
        for e in (-1, 0, 1):
            a = rng.integers(1, 5, size=TRACE_CHUNK * k + e)
            refs.append(a); queries.append(a.copy()); stripes.append((-2, 2))
    a = rng.integers(1, 5, size=400)
    b = np.concatenate([a[:100], rng.integers(1, 5, size=90), a[100:]])          # a 90-label insertion: the path crosses 90 diagonals
    refs += [a, b]; queries += [b, a]; stripes += [(-5, 100), (-100, 5)]
    got = _banded(refs, queries, stripes, P.EMBOSS, True)
    wants = _check(refs, queries, stripes, P.EMBOSS, True, got, "trace seams")
    assert wants[-1].gaps >= 90 and wants[-2].gaps >= 90


def test_a_long_thin_pair():
    rng = np.random.default_rng(20000)
    a = rng.integers(1, 5, size=20000)
    b = a.copy()
    b[rng.integers(0, 20000, size=600)] = rng.integers(1, 5, size=600)
    got = _banded([a], [b], [(-16, 16)], P.EMBOSS, True)
    _check([a], [b], [(-16, 16)], P.EMBOSS, True, got, "20000 x 20000")


def test_the_longest_reference_with_a_stripe_at_its_far_corner():
    rng = np.random.default_rng(65535)
    a = rng.integers(1, 5, size=65535)
    b = a[-320:-20].copy()
    b[::17] = 1
    stripes = [(-65535 + 300 - 40, -65535 + 300 + 40)]
    for free in (True, False):
        got = _banded([a], [b], stripes, P.EMBOSS, free)
        want = _check([a], [b], stripes, P.EMBOSS, free, got, "65535 x 300")[0]
        assert want.status == 1 and want.matches > 250


# ------------------------------------------------------------------------------------------------------ 6. forms and arguments

def test_score_only_and_counts_only_equal_the_full_form():
    rng = np.random.default_rng(6)
    refs, queries, stripes = [], [], []
    for n in range(16):
        N, M = int(rng.integers(0, 700)), int(rng.integers(0, 700))
        a, b = random_pair(rng, N, M, 4, n % 2 == 0)
        refs.append(a); queries.append(b); stripes.append(random_stripe(rng, N, M, 600))
    for free in (True, False):
        full = _banded(refs, queries, stripes, P.EMBOSS, free, max_band=600)
        _check(refs, queries, stripes, P.EMBOSS, free, full, "full form")
        counts = _banded(refs, queries, stripes, P.EMBOSS, free, max_band=600, return_ops=False)
        assert counts[3] is None and counts[4] is None
        for k in (0, 1, 2, 5):
            assert_equal_arrays(counts[k], full[k], "counts only, field %d" % k)
        score = _banded(refs, queries, stripes, P.EMBOSS, free, max_band=600, score_only=True)
        assert score[2] is None and score[3] is None and score[5] is None
        assert_equal_arrays(score[0], full[0], "score only: status")
        assert_equal_arrays(score[1], full[1], "score only: score")


def test_edge_hits_are_zero_under_a_wide_stripe_and_count_under_a_tight_one():
    rng = np.random.default_rng(7)
    a, b = random_pair(rng, 300, 300, 4, True)
    full = P.align(a, b, *P.EMBOSS, True)
    lo, hi = R.band_from_ops(full.ops)
    got = _banded([a, a, a], [b, b, b], [(lo - 1, hi + 1), (lo, hi), (lo + 1, hi)], P.EMBOSS, True)
    wants = _check([a, a, a], [b, b, b], [(lo - 1, hi + 1), (lo, hi), (lo + 1, hi)], P.EMBOSS, True, got, "edge hits")
    assert got[5][0] == 0 and got[5][1] >= 2 and wants[2].edge_hits > 0 and wants[2].score < full.score


def test_values_past_the_lengths_are_never_read():
    rng = np.random.default_rng(8)
    refs, queries, stripes = [], [], []
    for n in range(8):
        N, M = int(rng.integers(0, 90)), int(rng.integers(0, 90))
        a, b = random_pair(rng, N, M, 4, True)
        refs.append(a); queries.append(b); stripes.append(random_stripe(rng, N, M, 30))
    clean = _banded(refs, queries, stripes, P.EMBOSS, True, max_band=30, ref_width=120, query_width=130)
    dirty = _banded(refs, queries, stripes, P.EMBOSS, True, max_band=30, ref_width=120, query_width=130, fill=3)
    _check(refs, queries, stripes, P.EMBOSS, True, clean, "clean")
    for k in range(6):
        assert_equal_arrays(dirty[k], clean[k], "garbage past the lengths, field %d" % k)


def test_bad_rows_poison_only_their_own_row():
    rng = np.random.default_rng(9)
    refs, queries = zip(*[random_pair(rng, 50, 45, 4, True) for _ in range(6)])
    a, an = _pad(refs)
    b, bn = _pad(queries)
    an, bn = an.clone(), bn.clone()
    lo = torch.full((6,), -8, dtype=torch.int32)
    hi = torch.full((6,), 8, dtype=torch.int32)
    an[0] = 51; bn[1] = -1; lo[2], hi[2] = 3, 2; lo[3], hi[3] = -9, 8                 # each kind: a length above, one below, lo > hi, too wide
    W = _W()
    out = W.banded_align(a.to(DEV), an.to(DEV), b.to(DEV), bn.to(DEV), lo.to(DEV), hi.to(DEV), 17)
    got = _host(out)
    with pytest.raises(RuntimeError, match="banded_align.*4 pair"):
        W.check_device_flags()
    for n in range(4):
        assert got[0][n] == -1 and got[1][n] == INT_MIN and (got[2][n] == -1).all() and got[4][n] == 0 and not got[3][n].any() and got[5][n] == -1, n
    _check(refs[4:], queries[4:], [(-8, 8)] * 2, P.EMBOSS, True, [None if g is None else g[4:] for g in got], "beside bad rows")


def test_int64_int32_and_strided_rows():
    rng = np.random.default_rng(10)
    refs, queries = zip(*[random_pair(rng, 60, 64, 4, True) for _ in range(5)])
    stripes = [(-6, 10)] * 5
    want = _banded(refs, queries, stripes, P.EMBOSS, True)
    a, an = _pad(refs)
    b, bn = _pad(queries)
    lo, hi = torch.full((5,), -6), torch.full((5,), 10)
    W = _W()
    got = _host(W.banded_align(a.long().to(DEV), an.long().to(DEV), b.long().to(DEV), bn.tolist(), lo.to(DEV), hi.tolist(), 17))
    for k in range(6):
        assert_equal_arrays(got[k], want[k], "int64, field %d" % k)
    got = _host(W.banded_align(strided(a.numpy(), False), an.to(DEV), strided(b.numpy(), False), bn.to(DEV), lo.int().to(DEV), hi.int().to(DEV), 17))
    for k in range(6):
        assert_equal_arrays(got[k], want[k], "strided, field %d" % k)


def test_two_runs_are_bitwise_identical_and_a_graph_replays_them():
    rng = np.random.default_rng(11)
    refs, queries, stripes = [], [], []
    for n in range(12):
        N, M = int(rng.integers(200, 900)), int(rng.integers(200, 900))
        a, b = random_pair(rng, N, M, 4, True)
        refs.append(a); queries.append(b); stripes.append(random_stripe(rng, N, M, 700))
    a, an = _pad(refs)
    b, bn = _pad(queries)
    args = [t.to(DEV) for t in (a, an, b, bn)] + [torch.tensor([s[k] for s in stripes], dtype=torch.int32, device=DEV) for k in (0, 1)]
    W = _W()
    flat = lambda o: tuple(o.alignment) + (o.status, o.edge_hits)    # noqa: E731
    first, second = flat(W.banded_align(*args, 700)), flat(W.banded_align(*args, 700))
    assert all(torch.equal(u, v) for u, v in zip(first, second))
    graph, captured = capture(lambda: W.banded_align(*args, 700))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(flat(captured), first))
    _check(refs, queries, stripes, P.EMBOSS, True, _host(captured), "captured")
    W.check_device_flags()


def test_cpu_tensors_and_bad_arguments_raise():
    W = _W()
    a, an = _pad([[1, 2, 3]])
    lo = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        W.banded_align(a, an, a, an, lo, lo, 1)                      # host rows
    g = a.to(DEV)
    for bad in (0, 2049, 1.5, True, None):
        with pytest.raises(ValueError, match="max_band"):
            W.banded_align(g, an, g, an, lo, lo, bad)
    with pytest.raises(ValueError, match="diag_lo"):
        W.banded_align(g, an, g, an, torch.zeros(2, dtype=torch.int32, device=DEV), lo, 1)
    with pytest.raises(ValueError, match="65535"):
        W.banded_align(torch.zeros(1, 65536, dtype=torch.int32, device=DEV), an, g, an, lo, lo, 1)
    with pytest.raises(ValueError):
        W.band_from_ops(W.pairwise_align(g, an, g, an, return_ops=False))
    with pytest.raises(ValueError, match="margin"):
        W.band_from_ops(W.pairwise_align(g, an, g, an), margin=-1)
    wide = W.banded_align(torch.zeros(1, 9000, dtype=torch.int32, device=DEV), an, torch.ones(1, 9000, dtype=torch.int32, device=DEV),
                          torch.tensor([9000]), lo, lo + 3, 4)       # beyond pairwise_align's 8192 query labels
    assert int(wide.status[0]) == 1 and int(wide.alignment.ops_len[0]) >= 9000
