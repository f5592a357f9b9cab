"""The inputs of tests/test_gpu_quality.py, built on the CPU from fixed seeds (numpy only), with the greedy path and the float64
reference of each (tests/ctc_quality_ref.py) computed once and shared: tests/test_ctc_quality_ref.py checks on these very
inputs that the share of bases whose Q lies within NEAR of a rounding boundary k + 0.5 is small enough for the GPU test to
leave them out of its exact comparison of `qual`."""
import functools

import numpy as np

from tests import ctc_decode_ref as DR
from tests import ctc_quality_ref as QR

B, C = 4, 5
LENGTHS = (1, 37, 256, 257, 1000)
NEAR = 1e-3                         # a reference Q this close to k + 0.5 may round either way in fp32
LONG_RUN = 700                      # frames of the single run of read 1 at T = 1000: it crosses any 256-frame tile


def peaked_logits(seed, T, batch=B):
    """'trained-looking' output: a random path of runs with dwells 1-12 (any class, the blank among them), a random margin
    per read and per run above unit noise -- small margins let the noise break a run.  Returns (x [batch, C, T] float32,
    input_lengths [batch] int64).
      read 1   at T = 1000 holds one run of LONG_RUN frames of class 2
      read 2   has T_b < T; its last run ends exactly at T_b, and the frames past T_b go on with the same class
      read 3   is all blank: an empty read"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(batch, C, T))
    lens = np.full(batch, T, dtype=np.int64)
    if T > 1 and batch > 2:
        lens[2] = T - max(1, T // 10)
    for b in range(batch):
        margin = rng.uniform(2.0, 12.0)
        t, long_done = 0, False
        while t < T:
            c, d = int(rng.integers(0, C)), int(rng.integers(1, 13))
            top = margin * rng.uniform(0.6, 1.0)
            if b == 1 and T >= LONG_RUN + 200 and t >= 100 and not long_done:
                c, d, top, long_done = 2, LONG_RUN, 9.0, True         # 9 above unit noise: no frame of it loses its argmax
            if b == 2 and t < lens[2] <= t + d:
                c, d = 1 + c % (C - 1), T - t                         # a base whose run reaches T_b, and goes on past it
            if b == 3:
                c, top = 0, 9.0
            x[b, c, t:t + d] += top
            t += d
    return x.astype(np.float32), lens


def random_logits(seed, T, batch=B):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(batch, C, T)) * 1.5).astype(np.float32)
    lens = np.array([T, max(T - 3, 0), T // 2, T][:batch] + [T] * max(0, batch - 4), dtype=np.int64)
    return x, lens


def _softmax64(x):
    z = x.astype(np.float64)
    z = np.exp(z - z.max(axis=1, keepdims=True))
    return z / z.sum(axis=1, keepdims=True)


# name -> (builder, seed, T, kind, stat, layout, qscale, qbias)
CASES = {}
for _T in LENGTHS:
    CASES["peaked_T%d" % _T] = (peaked_logits, 100 + _T, _T, "logits", "mean", "BCT", 1.0, 0.0)
    CASES["random_T%d" % _T] = (random_logits, 200 + _T, _T, "logits", "mean", "BCT", 1.0, 0.0)
CASES["peaked_T1000_best"] = (peaked_logits, 1100, 1000, "logits", "best", "BCT", 1.0, 0.0)
CASES["random_T257_best"] = (random_logits, 457, 257, "logits", "best", "BCT", 1.0, 0.0)
CASES["peaked_T257_probs"] = (peaked_logits, 357, 257, "probs", "mean", "BCT", 1.0, 0.0)
CASES["peaked_T257_log_probs"] = (peaked_logits, 357, 257, "log_probs", "mean", "BCT", 1.0, 0.0)
CASES["peaked_T256_btc"] = (peaked_logits, 356, 256, "logits", "mean", "BTC", 1.0, 0.0)
CASES["peaked_T1000_calibrated"] = (peaked_logits, 1100, 1000, "logits", "mean", "BCT", 0.7, 2.5)


class Case(object):
    """x [B, C, T] float32 in the form `kind` names, input_lengths, the greedy path of x and the reference on that path"""

    def __init__(self, name):
        build, seed, T, self.kind, self.stat, self.layout, self.qscale, self.qbias = CASES[name]
        self.name, self.T = name, T
        logits, self.input_lengths = build(seed, T)
        if self.kind == "probs":
            self.x = _softmax64(logits).astype(np.float32)
        elif self.kind == "log_probs":
            self.x = np.log(_softmax64(logits)).astype(np.float32)
        else:
            self.x = logits
        self.labels, self.frames, self.lengths = DR.greedy_decode_batch(self.x, input_lengths=self.input_lengths)
        self.ref = QR.batch_qualities(self.x, self.labels, self.frames, self.lengths, self.input_lengths, kind=self.kind,
                                      stat=self.stat, qscale=self.qscale, qbias=self.qbias)
        # D of the error bound: the largest max_c x - x_c of this case's input
        self.D = float((self.x.astype(np.float64).max(axis=1) - self.x.astype(np.float64).min(axis=1)).max())

    def valid(self):
        """[B, Lmax] bool: the entries that are bases"""
        return np.arange(self.labels.shape[1])[None, :] < self.lengths[:, None]

    def near_boundary(self):
        """[B, Lmax] bool: bases whose reference Q lies within NEAR of a rounding boundary k + 0.5"""
        q = self.ref["Q"]
        with np.errstate(invalid="ignore"):
            frac = q - np.floor(q)
            return self.valid() & np.isfinite(q) & (np.abs(frac - 0.5) <= NEAR)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def error_bound(D):
    """relative: the rounding of x - max in the exponent (D 2^-24 each way), a few ulp of expf, two C-term sums, a division"""
    return (2.0 * D + 2.0 * C + 16.0) * 2.0 ** -24
