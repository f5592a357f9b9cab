"""CPU: the C ABI of the signal alignment (csrc/wn_sigalign.hip): the exported symbols, the ctypes rows against the header argument
by argument, and every host-side rejection in its documented order (shape, unsupported, NULL, workspace), with fake pointers:
every call below returns before anything would be launched.  And the host arithmetic of signal_model against exact rationals."""
import ctypes
import math
from fractions import Fraction

import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

ALIGN = Entry("wn_signal_align", dict(signal=FAKE, signal_kind=0, signal_stride=1000, signal_lengths=FAKE, scale_shift=FAKE, labels=FAKE,
                                      labels_stride=100, label_lengths=FAKE, model=FAKE, batch=2, max_signal=1000, max_labels=100, max_events=96,
                                      k=5, first=0, frac_bits=12, weight_shift=40, max_cost=2 ** 31 - 1, band=64, starts=FAKE, score=FAKE,
                                      band_hits=FAKE, sample_state=FAKE, workspace=FAKE, workspace_bytes=0, bad=None,
                                      stream=None))                  # workspace_bytes 0: never launches
SIZE = Entry("wn_signal_align_workspace_bytes", dict(batch=2, max_signal=1000, band=64))


def test_symbols_are_exported(lib):
    ALIGN.check_exported(lib)
    SIZE.check_exported(lib)


def test_signature_rows_match_the_header():
    ALIGN.check_declared()                                           # 27 arguments
    SIZE.check_declared()                                            # 3


def test_workspace_size(lib):
    size = lib.wn_signal_align_workspace_bytes
    for args in ((0, 10, 64), (-1, 10, 64), (65536, 10, 64), (1, 0, 64), (1, 2 ** 24 + 1, 64), (1, 10, 0), (1, 10, 32), (1, 10, 96),
                 (1, 10, 2112), (1, 10, -64)):
        assert size(*args) == 0, args
    assert size(65535, 1, 64) > 0 and size(1, 2 ** 24, 2048) == 2 ** 24 * 256
    for B, L, W in ((1, 1, 64), (3, 129, 576), (32, 17001, 512), (2, 1000, 64)):
        assert B * L * W // 8 <= size(B, L, W) < B * L * W // 8 + 16 and size(B, L, W) % 16 == 0       # one bit per sample and slot


def test_rejects_on_the_host_in_order(lib):
    assert ALIGN(lib) == WN_ERR_WORKSPACE                            # everything else about the default call is accepted
    ALIGN.rejects(lib, "signal",
                  shape=(dict(batch=0), dict(batch=-2), dict(max_signal=0), dict(max_signal=-5), dict(max_labels=0), dict(max_events=0),
                         dict(max_events=-1), dict(signal_stride=-1), dict(labels_stride=-1), dict(signal_kind=2), dict(signal_kind=-1)),
                  unsupported=(dict(k=0), dict(k=7), dict(first=-1), dict(first=9), dict(frac_bits=-1), dict(frac_bits=21), dict(weight_shift=15),
                               dict(weight_shift=64), dict(max_cost=0), dict(max_cost=-1), dict(band=0), dict(band=32), dict(band=96),
                               dict(band=2112), dict(band=-64), dict(batch=65536), dict(max_signal=2 ** 24 + 1), dict(max_events=2 ** 20 + 1)),
                  accepted=(dict(k=1), dict(k=6), dict(first=0), dict(first=8), dict(frac_bits=0), dict(frac_bits=20), dict(weight_shift=16),
                            dict(weight_shift=63), dict(max_cost=1), dict(max_cost=2 ** 31 - 1), dict(band=64), dict(band=128), dict(band=576),
                            dict(band=2048), dict(batch=65535), dict(batch=1), dict(max_signal=2 ** 24), dict(max_events=2 ** 20),
                            dict(signal_kind=1), dict(signal_stride=0, labels_stride=0)),
                  required=("signal", "signal_lengths", "labels", "label_lengths", "model", "starts", "score", "band_hits", "workspace"))
    for name in ("scale_shift", "sample_state", "bad"):              # optional
        assert ALIGN(lib, **{name: None}) == WN_ERR_WORKSPACE, name
    # the workspace: too small by one byte, misaligned, and a signal off its element size
    need = SIZE(lib)
    assert need == 16000
    assert ALIGN(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert ALIGN(lib, workspace=ctypes.c_void_p((1 << 20) + 8), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert ALIGN(lib, signal=ctypes.c_void_p((1 << 20) + 2), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert ALIGN(lib, signal=ctypes.c_void_p((1 << 20) + 1), signal_kind=1, workspace_bytes=need) == WN_ERR_WORKSPACE
    assert ALIGN(lib, band=128, workspace_bytes=need) == WN_ERR_WORKSPACE            # the size follows the band
    # the order: shape, then unsupported, then NULL, then workspace
    assert ALIGN(lib, batch=0, k=7, signal=None) == WN_ERR_BAD_SHAPE
    assert ALIGN(lib, signal_kind=2, band=96, model=None) == WN_ERR_BAD_SHAPE
    assert ALIGN(lib, max_events=0, batch=65536, workspace=None) == WN_ERR_BAD_SHAPE
    assert ALIGN(lib, k=7, signal=None) == WN_ERR_UNSUPPORTED
    assert ALIGN(lib, weight_shift=64, score=None) == WN_ERR_UNSUPPORTED
    assert ALIGN(lib, batch=65536, workspace=None) == WN_ERR_UNSUPPORTED
    assert ALIGN(lib, model=None, workspace_bytes=0) == WN_ERR_NULL


# ---- signal_model: the host-side integer table
def _exact_rows(means, stdvs, F, cb):
    """(S, rows) by the documented rule in exact rationals; the offset's logarithm in float64"""
    sq = [Fraction(float(s)) * 2 ** F for s in stdvs]
    w = lambda S, s: round(Fraction(2 ** (S + cb)) / (2 * s * s))    # noqa: E731
    S = max(S for S in range(16, 64) if w(S, min(sq)) < 2 ** 31)
    return S, [[round(Fraction(float(m)) * 2 ** F), w(S, s), round(2 ** cb * math.log(float(s)))] for m, s in zip(means, sq)]


def test_signal_model_against_exact_rationals():
    import wavenet_speech_amd as W
    from wavenet_speech_amd import synthetic
    means, stdvs = synthetic.standin_kmer_table()
    model = W.signal_model(means, stdvs)
    S, rows = _exact_rows(means.tolist(), stdvs.tolist(), 12, 8)
    assert (model.k, model.frac_bits, model.cost_bits, model.weight_shift) == (5, 12, 8, S)
    assert model.table.dtype == torch.int32 and model.table.tolist() == rows
    top = max(r[1] for r in rows)
    assert 2 ** 29 <= top < 2 ** 31 and min(r[1] for r in rows) >= 1
    # the cost it stands for: (q - level)^2 weight >> S is 2^cost_bits d^2 / (2 s^2) to within the rounding of the weight and one floor
    s, (level, weight, _) = float(stdvs[7]) * 4096, rows[7]
    for d in (1, 100, 5000, 40000):
        exact = 256 * d * d / (2 * s * s)
        assert abs(((d * d * weight) >> S) - exact) <= 1 + exact * 2.0 ** -28
    # the choice of S moves with the smallest stdv and with frac_bits and cost_bits; ties round to even
    for stdv, F, cb in ((0.5, 12, 8), (3.0, 12, 8), (1.0, 0, 0), (1.0, 20, 16), (0.1, 0, 8), (300.0, 12, 8)):
        m = W.signal_model([0.0, 1.5, -2.5, 7.0], [stdv, 2 * stdv, 3 * stdv, 5 * stdv], frac_bits=F, cost_bits=cb)
        S, rows = _exact_rows([0.0, 1.5, -2.5, 7.0], [stdv, 2 * stdv, 3 * stdv, 5 * stdv], F, cb)
        assert m.weight_shift == S and m.table.tolist() == rows and m.k == 1, (stdv, F, cb)
        assert S == 63 or 2 ** 30 - 1 <= rows[0][1] < 2 ** 31
    assert W.signal_model([0.5, 1.5, 2.5, -0.5], [1.0] * 4, frac_bits=0).table[:, 0].tolist() == [0, 2, 2, 0]
    # what fit_kmer_model returns goes straight in (with a prior: no NaN)
    stats = torch.zeros(4, 5, dtype=torch.int64)
    stats[0] = torch.tensor([10, 200, 200 * 4096 * 3, (200 * (4096 * 3) ** 2 + 200 * 4096 ** 2) & 0xffffffff, (200 * (4096 * 3) ** 2 + 200 * 4096 ** 2) >> 32])
    fit = W.fit_kmer_model(stats, prior=([1.0, 2.0, 3.0, 4.0], [1.0, 1.0, 1.0, 1.0]))
    m = W.signal_model(fit[0], fit[1])
    assert m.table[0, 0] == 3 * 4096 and m.table[:, 1].tolist() == [m.table[0, 1]] * 4
    with pytest.raises(ValueError, match="prior"):
        W.signal_model(*W.fit_kmer_model(stats)[:2])


def test_signal_model_refusals_and_hand_filled_tables():
    import wavenet_speech_amd as W
    ok_m, ok_s = [1.0, 2.0, 3.0, 4.0], [1.0, 1.0, 2.0, 1.0]
    for means, stdvs in ((ok_m, [1.0, 0.0, 1.0, 1.0]), (ok_m, [1.0, -1.0, 1.0, 1.0]), (ok_m, [1.0, float("nan"), 1.0, 1.0]),
                         (ok_m, [1.0, float("inf"), 1.0, 1.0]), ([1.0, float("nan"), 3.0, 4.0], ok_s), ([1.0, float("inf"), 3.0, 4.0], ok_s),
                         (ok_m, [1.0, 1.0, 1.0]), (ok_m[:3], ok_s[:3]), ([3000.0, 0.0, 0.0, 0.0], ok_s)):
        with pytest.raises(ValueError):
            W.signal_model(means, stdvs)
    W.signal_model([2047.99, 0.0, 0.0, 0.0], ok_s)                   # the level just inside 2^23
    with pytest.raises(ValueError, match="weight below 1"):          # stdvs 2^16 apart: the smaller weight is 2^-32 of the larger
        W.signal_model(ok_m, [1.0, 1.0, 1.0, 70000.0])
    W.signal_model(ok_m, [1.0, 1.0, 1.0, 20000.0])
    with pytest.raises(ValueError, match="too small"):               # the largest weight does not fit at S = 16
        W.signal_model(ok_m, [1e-3, 1.0, 1.0, 1.0], frac_bits=0, cost_bits=16)
    with pytest.raises(ValueError):
        W.signal_model(ok_m, ok_s, frac_bits=21)
    # a table filled by hand comes back as it went in; the ranges are checked
    rows = [[10, 1 << 16, 0], [20, 1, -5], [-(2 ** 23) + 1, 2 ** 31 - 1, 2 ** 30 - 1], [2 ** 23 - 1, 7, -(2 ** 30) + 1]]
    m = W.SignalModel(torch.tensor(rows), 16, frac_bits=0, cost_bits=0)
    assert m.table.tolist() == rows and m.table.dtype == torch.int32 and (m.k, m.weight_shift, m.frac_bits, m.cost_bits) == (1, 16, 0, 0)
    again = W.SignalModel(m.table, m.weight_shift, m.frac_bits, m.cost_bits)
    assert again.table.tolist() == rows
    for r, c, v in ((0, 1, 0), (0, 1, 2 ** 31), (0, 0, 2 ** 23), (0, 0, -(2 ** 23)), (0, 2, 2 ** 30), (0, 2, -(2 ** 30))):
        broken = torch.tensor(rows)
        broken[r, c] = v
        with pytest.raises(ValueError):
            W.SignalModel(broken, 16)
    for shift in (15, 64):
        with pytest.raises(ValueError):
            W.SignalModel(torch.tensor(rows), shift)
    with pytest.raises(ValueError):
        W.SignalModel(torch.tensor(rows[:3]), 16)
    with pytest.raises(ValueError):
        W.SignalModel(torch.tensor(rows).double(), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.signal_align(torch.zeros(1, 10), [10], torch.ones(1, 5, dtype=torch.int32), [5], m)
