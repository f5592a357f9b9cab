"""CPU: the numpy restatement of the radix selection (tests/read_stats_ref.py) against np.sort, np.median and np.quantile, on
the inputs of the GPU tests (tests/read_stats_cases.py) plus every rank of small random reads."""
import numpy as np
import pytest

from tests import read_stats_cases as C
from tests import read_stats_ref as R

LINEAR_BOUND = 2.0 ** -22          # one fp32 rounding plus numpy's differently ordered lerp, relative to the read's largest magnitude


def _same(got, want):
    np.testing.assert_array_equal(np.float32(got), np.float32(want))           # NaN equals NaN, -0.0 equals +0.0


def _batches():
    yield "ragged_int16", C.ragged("int16")
    yield "ragged_float32", C.ragged("float32")
    yield "int16_patterns", C.int16_patterns()[1:]
    yield "fp32_patterns", C.fp32_patterns()[1:]


def test_keys_preserve_the_order():
    x = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf, np.nan], dtype=np.float32)
    k, bits = R.keys(x)
    assert bits == 32 and np.all(np.diff(k.astype(np.int64)) > 0)              # -0.0 directly below +0.0, NaN above +inf
    assert int(k[4]) - int(k[3]) == 1
    for v, key in zip(x, k):
        _same(R.value_of_key(key, np.float32, False), v)
    y = np.array([-32768, -1, 0, 1, 32767], dtype=np.int16)
    k, bits = R.keys(y)
    assert bits == 16 and list(k) == [0, 0x7FFF, 0x8000, 0x8001, 0xFFFF]
    for v, key in zip(y, k):
        _same(R.value_of_key(key, np.int16, False), v)
    d, bits = R.keys(y, center=np.float32(0.5))
    assert bits == 32 and list(d.view(np.float32)) == [32768.5, 1.5, 0.5, 0.5, 32766.5]


def test_one_pass_of_the_selection():
    k = np.array([0x0102, 0x0103, 0x0203, 0x0203, 0xFF00], dtype=np.uint32)
    key, trace = R.select_key(k, 16, 3)
    assert key == 0x0203
    (p0, h0, d0, r0), (p1, h1, d1, r1) = trace
    assert p0 == 0 and h0[1] == 2 and h0[2] == 2 and h0[255] == 1 and h0.sum() == 5 and d0 == 2 and r0 == 1     # 3 - the two in bin 1
    assert p1 == 2 and h1[3] == 2 and h1.sum() == 2 and d1 == 3 and r1 == 1


@pytest.mark.parametrize("name", ["ragged_int16", "ragged_float32", "int16_patterns", "fp32_patterns"])
def test_order_statistics_equal_sort(name):
    x, lengths = dict(_batches())[name]
    want = C.sorted_reads(x, lengths)
    for K, seed in ((8, 11), (1, 12)):
        ranks = C.edge_ranks(lengths, K, seed)
        got = np.array([[R.order_statistic(x[b], int(lengths[b]), int(r)) for r in ranks[b]] for b in range(len(lengths))])
        _same(got, C.pick(want, ranks))


@pytest.mark.parametrize("name", ["ragged_int16", "ragged_float32"])
def test_deviation_mode_equals_sort_of_float32_deviations(name):
    x, lengths = dict(_batches())[name]
    centers = C.deviation_centers(x.dtype, len(lengths))
    want = C.sorted_reads(x, lengths, centers)
    ranks = C.edge_ranks(lengths, 8, 13)
    got = np.array([[R.order_statistic(x[b], int(lengths[b]), int(r), centers[b]) for r in ranks[b]] for b in range(len(lengths))])
    _same(got, C.pick(want, ranks))


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_every_rank_of_small_reads(dtype):
    rng = np.random.default_rng(14)
    for n in list(range(1, 18)) + [31, 32, 33, 63, 64]:
        x = rng.integers(-40, 40, n + 3).astype(dtype) if rng.integers(0, 2) else \
            (rng.integers(-32768, 32768, n + 3).astype(dtype) if dtype == np.int16 else rng.normal(0, 5, n + 3).astype(dtype))
        want = np.sort(x[:n])
        c = np.float32(rng.choice([0.0, 0.5, 1.37]))
        wantd = np.sort(np.abs(x[:n].astype(np.float32) - c))
        for r in range(n):
            _same(R.order_statistic(x, n, r), want[r])
            _same(R.order_statistic(x, n, r, c), wantd[r])
        for r in (-1, n):
            assert R.order_statistic(x, n, r) == 0.0                           # refused
    assert R.order_statistic(np.zeros(4, np.int16), 5, 0) == 0.0 and R.order_statistic(np.zeros(4, np.int16), -1, 0) == 0.0


def test_med_mad_of_int16_equals_float64_numpy():
    for x, lengths in (C.ragged("int16"), C.int16_patterns()[1:]):
        for b, n in enumerate(int(v) for v in lengths):
            med, mad = R.med_mad(x[b], n)
            r = x[b, :n].astype(np.float64)
            assert np.float64(med) == np.median(r) and np.float64(mad) == np.median(np.abs(r - np.median(r))), (b, n)
    med, mad = R.med_mad(np.array([7, 9], dtype=np.int16), 1)
    assert med == 7.0 and mad == 0.0
    assert R.medmad_normalisation(np.array([7, 9], dtype=np.int16), 1) == (1.0, -7.0)


def test_med_mad_of_fp32_is_the_midpoint_rule():
    x, lengths = C.ragged("float32")
    for b, n in enumerate(int(v) for v in lengths):
        s = np.sort(x[b, :n])
        med = np.float32(np.float32(s[(n - 1) // 2] + s[n // 2]) * np.float32(0.5))
        d = np.sort(np.abs(x[b, :n] - med))
        mad = np.float32(np.float32(d[(n - 1) // 2] + d[n // 2]) * np.float32(0.5))
        _same(R.med_mad(x[b], n), (med, mad))


@pytest.mark.parametrize("name", ["ragged_int16", "ragged_float32"])
def test_quantiles_against_numpy(name):
    x, lengths = dict(_batches())[name]
    for b, n in enumerate(int(v) for v in lengths):
        r = x[b, :n].astype(np.float64)
        top = np.abs(r).max()
        for q in (0.0, 0.2, 0.5, 0.9, 1.0, 0.3333):
            for method in ("lower", "higher", "midpoint"):
                assert np.float64(R.quantile(x[b], n, q, method)) == np.float32(np.quantile(r, q, method=method)), (b, n, q, method)
            got, want = np.float64(R.quantile(x[b], n, q)), np.quantile(r, q)
            assert abs(got - want) <= LINEAR_BOUND * top, (b, n, q, got, want)
    pos, lo, hi = R.quantile_ranks(11, 0.25)
    assert (pos, lo, hi) == (2.5, 2, 3) and R.quantile_ranks(11, 0.5)[1:] == (5, 5) and R.quantile_ranks(1, 0.9)[1:] == (0, 0)
