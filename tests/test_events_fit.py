"""CPU: the host side of the event tables (wavenet_speech_amd/events.py): fit_kmer_model against the exact rational, fit_dwell_model
against an independent bisection of the same likelihood equation, and the eventalign formatter's exact text.

Bounds.  fit_kmer_model divides exact integers once: the mean carries one float64 rounding, the stdv two (the division and the
square root), so 1e-12 relative is far above both.  fit_dwell_model solves log a - digamma(a) = s: the bisection here brackets the
same root with scipy's digamma, and the two agree to 1e-8 relative when both residuals are below 1e-10 (the function's slope in
log a is between -1 and -1/2)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.special import digamma

from wavenet_speech_amd import events as E
from wavenet_speech_amd.synthetic import _dwell_spec


def _stats_table(rng, rows, frac_bits):
    """kmer_stats of `rows` k-mers from integer samples, with every sum formed in Python integers; also the samples"""
    table, samples = [], []
    for i in range(rows):
        n = int(rng.integers(0, 400))
        level, spread = rng.uniform(-100.0, 120.0), rng.uniform(0.5, 6.0)
        q = [int(round(v * (1 << frac_bits))) for v in (level + spread * rng.standard_normal(n))]
        sizes, events, lo, hi, left = [], 0, 0, 0, q
        while left:                                                  # events of 1..9 samples: the limbs are taken per event
            m = int(rng.integers(1, 10))
            ev, left = left[:m], left[m:]
            s2 = sum(v * v for v in ev)
            lo, hi, events = lo + (s2 & 0xffffffff), hi + (s2 >> 32), events + 1
        table.append([events, n, sum(q), lo, hi])
        samples.append(q)
    return table, samples


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@pytest.mark.parametrize("frac_bits", [0, 12, 20])
def test_fit_kmer_model_against_the_exact_rational(frac_bits):
    rng = np.random.default_rng(3 + frac_bits)
    table, samples = _stats_table(rng, 64, frac_bits)
    table[5] = [1, 65536, 65536 * 8388607, (65536 * 8388607 ** 2) & 0xffffffff, (65536 * 8388607 ** 2) >> 32]      # the largest event
    samples[5] = [8388607] * 65536
    means, stdvs, counts = E.fit_kmer_model(torch.tensor(table, dtype=torch.int64), frac_bits=frac_bits, min_count=100)
    assert means.dtype == stdvs.dtype == counts.dtype == torch.float64 and means.shape == stdvs.shape == counts.shape == (64,)
    used = 0
    for i, q in enumerate(samples):
        n = len(q)
        assert counts[i] == n
        if n < 100:
            assert math.isnan(means[i]) and math.isnan(stdvs[i])
            continue
        used += 1
        mean = Fraction(sum(q), n << frac_bits)                      # independently: straight from the samples
        var = Fraction(sum((Fraction(v, 1 << frac_bits) - mean) ** 2 for v in q), n)
        assert _rel(float(means[i]), float(mean)) <= 1e-12, i
        want = math.sqrt(var) if var else 0.0
        assert (float(stdvs[i]) == 0.0) if var == 0 else (_rel(float(stdvs[i]), want) <= 1e-12), i
    assert used > 20 and float(stdvs[5]) == 0.0 and float(means[5]) == 8388607 / (1 << frac_bits)


def test_fit_kmer_model_prior_and_min_count():
    table = [[3, 9, 90, 900, 0], [50, 100, 1000, 10400, 0], [1, 99, 0, 0, 0], [0, 0, 0, 0, 0]]
    prior = (torch.arange(4.0), 10.0 + torch.arange(4.0))
    means, stdvs, counts = E.fit_kmer_model(np.array(table), frac_bits=0, min_count=100, prior=prior)
    assert means.tolist() == [0.0, 10.0, 2.0, 3.0] and counts.tolist() == [9.0, 100.0, 99.0, 0.0]
    assert stdvs.tolist() == [10.0, 2.0, 12.0, 13.0]                 # 10400 / 100 - 10^2 = 4
    means, stdvs, _ = E.fit_kmer_model(table, frac_bits=0, min_count=9)
    assert means[0] == 10.0 and stdvs[0] == 0.0 and means[1] == 10.0 and math.isnan(means[3]) and math.isnan(stdvs[3])
    assert E.fit_kmer_model(table, frac_bits=1, min_count=1)[0][1] == 5.0
    for wrong in (dict(kmer_stats=[[1, 2, 3, 4]]), dict(kmer_stats=table, min_count=0), dict(kmer_stats=table, frac_bits=21),
                  dict(kmer_stats=table, prior=(torch.zeros(3), torch.zeros(3))), dict(kmer_stats=torch.zeros(4, 5))):
        with pytest.raises(ValueError):
            E.fit_kmer_model(**wrong)


def _bisect_shape(s):
    lo, hi = 1e-6, 1e9                                               # log a - digamma(a) falls from +inf to 0
    for _ in range(400):
        mid = math.sqrt(lo * hi)
        if math.log(mid) - float(digamma(mid)) > s:
            lo = mid
        else:
            hi = mid
    return math.sqrt(lo * hi)


def _hist_stats(hist):
    n = sum(hist)
    mean = Fraction(sum(d * h for d, h in enumerate(hist)), n)
    mean_log = math.fsum(h * math.log(d) for d, h in enumerate(hist) if h) / n
    return float(mean), math.log(mean) - mean_log


@pytest.mark.parametrize("shape, rate", [(2.461964, 587.2858), (0.7, 100.0), (30.0, 6000.0)])
def test_fit_dwell_model_against_bisection(shape, rate):
    rng = np.random.default_rng(11)
    sample_rate, D = 4000.0, 1023
    d = np.maximum(1, (rng.gamma(shape, 1.0 / rate, size=(16, 4000)) * sample_rate).astype(np.int64))
    assert d.max() < D
    hist = np.stack([np.bincount(row, minlength=D + 1) for row in d])
    kind, a, r, sr = E.fit_dwell_model(torch.from_numpy(hist), sample_rate)
    assert kind == "gamma" and sr == sample_rate and _dwell_spec((kind, a, r, sr))[0] == 2          # what ragged_reads takes
    mean, s = _hist_stats(hist.sum(0).tolist())
    want = _bisect_shape(s)
    print("shape %.10g (bisection %.10g), rate %.10g, residual %.3e" % (a, want, r, abs(math.log(a) - float(digamma(a)) - s)))
    assert abs(math.log(a) - float(digamma(a)) - s) <= 1e-10
    assert _rel(a, want) <= 1e-8 and _rel(r, want * sample_rate / mean) <= 1e-8
    per = E.fit_dwell_model(hist, sample_rate, per_kmer=True, min_count=4000)
    assert per.shape == (16, 2) and per.dtype == torch.float64
    for i in (0, 15):
        mean_i, s_i = _hist_stats(hist[i].tolist())
        assert _rel(float(per[i, 0]), _bisect_shape(s_i)) <= 1e-8 and _rel(float(per[i, 1]), _bisect_shape(s_i) * sample_rate / mean_i) <= 1e-8
    assert torch.isnan(E.fit_dwell_model(hist, sample_rate, per_kmer=True, min_count=4001)).all()


def test_fit_dwell_model_refusals():
    hist = np.zeros((4, 11), dtype=np.int64)
    hist[0, 3], hist[1, 5], hist[2, 4] = 60, 50, 40
    assert E.fit_dwell_model(hist, 4000.0)[0] == "gamma"
    clamped = hist.copy()
    clamped[3, 10] = 1
    with pytest.raises(ValueError, match="clamp column"):
        E.fit_dwell_model(clamped, 4000.0)
    with pytest.raises(ValueError, match="clamp column"):
        E.fit_dwell_model(clamped, 4000.0, per_kmer=True)
    with pytest.raises(ValueError, match="min_count"):
        E.fit_dwell_model(hist, 4000.0, min_count=151)
    one_length = np.zeros((2, 11), dtype=np.int64)
    one_length[:, 6] = 500
    with pytest.raises(ValueError, match="same length"):
        E.fit_dwell_model(one_length, 4000.0)
    assert torch.isnan(E.fit_dwell_model(one_length, 4000.0, per_kmer=True)).all()
    for wrong in (dict(sample_rate=0.0), dict(sample_rate=float("inf")), dict(sample_rate=4000.0, min_count=0)):
        with pytest.raises(ValueError):
            E.fit_dwell_model(hist, **wrong)


def _small_events():
    i32, i64 = torch.int32, torch.int64
    kmer = torch.tensor([[-1, 1 * 4 + 2, 2 * 4 + 0], [3 * 4 + 3, -2, -4]], dtype=i32)
    start = torch.tensor([[0, 2, 5], [0, 4, 0]], dtype=i32)
    length = torch.tensor([[2, 3, 2], [4, 0, 0]], dtype=i32)
    # frac_bits 2: samples (q / 4).  event (0, 1): 10, 11, 12 -> q 40 44 48; (0, 2): 7.25 7.75; (1, 0): four times 100.5
    total = torch.tensor([[0, 132, 60], [1608, 0, 0]], dtype=i64)
    squares = torch.tensor([[0, 40 * 40 + 44 * 44 + 48 * 48, 29 * 29 + 31 * 31], [4 * 402 * 402, 0, 0]], dtype=i64)
    return E.KmerEvents(kmer, start, length, total, squares, None, None, None, k=2, first=0, frac_bits=2, max_dwell=255)


def test_event_levels_from_the_integer_sums():
    ev = _small_events()
    mean, stdv = ev.mean, ev.stdv
    assert mean.dtype == torch.float64 and mean[0, 1] == 11.0 and mean[0, 2] == 7.5 and mean[1, 0] == 100.5
    assert torch.isnan(mean[0, 0]) and torch.isnan(mean[1, 1]) and torch.isnan(mean[1, 2]) and torch.isnan(stdv[0, 0])
    assert abs(float(stdv[0, 1]) - math.sqrt(2.0 / 3.0)) <= 1e-12 and stdv[0, 2] == 0.25 and stdv[1, 0] == 0.0


def test_eventalign_rows_exact_text():
    ev = _small_events()
    labels = torch.tensor([[1, 2, 3, 1], [4, 4, 4, 0]])
    rows = E.eventalign_rows(ev, labels)
    assert rows == ["read_index\tposition\treference_kmer\tevent_index\tevent_level_mean\tevent_stdv\tevent_length\tevent_start_time",
                    "0\t1\tGC\t1\t11.00\t0.816\t3\t2",
                    "0\t2\tCA\t2\t7.50\t0.250\t2\t5",
                    "1\t0\tTT\t0\t100.50\t0.000\t4\t0"]
    model = (torch.arange(16.0) + 5.0, torch.full((16,), 2.0))
    rows = E.eventalign_rows(ev, labels, names=["r-a", "r-b"], model=model, sample_rate=4000.0, header=False)
    assert rows == ["r-a\t1\tGC\t1\t11.00\t0.816\t0.00075\t0.00050\t11.00\t2.00\t0.00",
                    "r-a\t2\tCA\t2\t7.50\t0.250\t0.00050\t0.00125\t13.00\t2.00\t-2.75",
                    "r-b\t0\tTT\t0\t100.50\t0.000\t0.00100\t0.00000\t20.00\t2.00\t40.25"]
    assert E.eventalign_rows(ev, labels, model=model)[0].split("\t") == list(E.EVENTALIGN_COLUMNS)
    assert E.eventalign_rows(ev, labels, alphabet=" ACGT", header=False)[0].split("\t")[2] == "CG"
    with pytest.raises(ValueError):
        E.eventalign_rows(ev, labels, names=["one"])
    with pytest.raises(ValueError):
        E.eventalign_rows(ev._replace(kmer=None), labels)
