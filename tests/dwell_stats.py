"""The yardstick for random dwell times: Pearson's chi-square of a sample against the EXACT pmf of the reference's formulas.
tests/test_ragged_reads.py holds it to numpy draws of those formulas (it accepts them, and rejects slightly different ones);
tests/test_gpu_reads.py applies the same function to the device's draws.

    uniform   np.random.randint(max(r - w, 1), r + w): every integer of the interval equally likely
    gamma     max(1, int(g * srate)), g ~ Gamma(shape, scale 1 / rate):  P(k) = F((k + 1) / srate) - F(k / srate) with
              F(x) = gammainc(shape, rate * x) in float64, the zero bin folded into 1

Bins whose expectation is below 5 are merged with their neighbours; a draw outside the pmf's support rejects at once.  The
bound is the 1 - 1e-6 quantile of chi-square by Wilson-Hilferty: a correct generator fails one run in a million, and with
200 000 draws a 5 % error in the gamma's shape overshoots it many times (the CPU test shows both)."""
import math

import torch

Z_1E6 = 4.753424308822899            # the 1 - 1e-6 quantile of the standard normal


def uniform_pmf(r, w):
    """(first value, probabilities) of the integer drawn uniformly from [max(r - w, 1), r + w)"""
    lo, hi = max(r - w, 1), r + w
    return lo, torch.full((hi - lo,), 1.0 / (hi - lo), dtype=torch.float64)


def gamma_floor_pmf(shape, rate, srate, tail=1e-13):
    """(1, probabilities of 1, 2, ...) of max(1, floor(g * srate)); the support is cut where the upper tail falls below `tail`
    and the last bin takes that tail"""
    a = torch.tensor(shape, dtype=torch.float64)
    kmax = 2
    while float(torch.special.gammaincc(a, torch.tensor(rate * kmax / srate, dtype=torch.float64))) >= tail:
        kmax *= 2
    edges = torch.arange(0, kmax + 1, dtype=torch.float64) * (rate / srate)
    cdf = torch.special.gammainc(a, edges)
    p = cdf[1:] - cdf[:-1]                                       # P(floor = k), k = 0 .. kmax - 1
    p[1] += p[0]                                                 # the zero bin is folded into 1
    p = p[1:].clone()
    p[-1] += 1.0 - float(cdf[-1])
    return 1, p


def chi_square_quantile(dof, z=Z_1E6):
    """Wilson-Hilferty: chi2_dof is close to dof * (1 - 2 / (9 dof) + z * sqrt(2 / (9 dof)))^3"""
    c = 2.0 / (9.0 * dof)
    return dof * (1.0 - c + z * math.sqrt(c)) ** 3


def chi_square(samples, pmf):
    """(statistic, degrees of freedom, draws outside the support) of integer `samples` (any tensor) against pmf = (first, probs)"""
    first, probs = pmf
    x = samples.detach().cpu().flatten().long() - first
    n = x.numel()
    outside = int(((x < 0) | (x >= probs.numel())).sum())
    counts = torch.bincount(x.clamp(0, probs.numel() - 1), minlength=probs.numel()).double()
    expect = probs * n
    # merge runs of bins, front to back, until each merged bin expects at least 5; a short last run joins the one before it
    obs_m, exp_m, o, e = [], [], 0.0, 0.0
    for c, ex in zip(counts.tolist(), expect.tolist()):
        o, e = o + c, e + ex
        if e >= 5.0:
            obs_m.append(o)
            exp_m.append(e)
            o, e = 0.0, 0.0
    if e > 0.0 or o > 0.0:
        if exp_m:
            obs_m[-1] += o
            exp_m[-1] += e
        else:
            obs_m.append(o)
            exp_m.append(e)
    stat = sum((ob - ex) ** 2 / ex for ob, ex in zip(obs_m, exp_m))
    return stat, len(exp_m) - 1, outside


def accepts(samples, pmf):
    """True if the sample passes: nothing outside the support and the statistic under the 1 - 1e-6 quantile"""
    stat, dof, outside = chi_square(samples, pmf)
    return outside == 0 and dof >= 1 and stat <= chi_square_quantile(dof)
