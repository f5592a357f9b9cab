"""CPU: the C ABI of the event alignment (csrc/wn_eventalign.hip): the exported symbols, the ctypes rows against the header
argument by argument, the workspace function and every host-side rejection on both sides of its limit and in its documented order
(shape, unsupported, NULL, workspace), with fake pointers: every call below returns before anything would be launched.  And the
host side of the Python surface: move_costs against exact values, fit_moves, and event_align's refusals."""
import ctypes
import math

import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

ALIGN = Entry("wn_event_align", dict(n_events=FAKE, ev_starts=FAKE, ev_sum=FAKE, ev_sumsq=FAKE, labels=FAKE, labels_stride=100, label_lengths=FAKE,
                                     model=FAKE, batch=2, max_events=1000, max_labels=100, max_states=96, k=5, first=0, frac_bits=12,
                                     weight_shift=40, max_cost=2 ** 31 - 1, band=64, move_cost0=504, move_cost1=122, move_cost2=412, move_cost3=824,
                                     starts=FAKE, score=FAKE, event_state=FAKE, move_counts=FAKE, band_hits=FAKE, workspace=FAKE,
                                     workspace_bytes=0, bad=None, stream=None))      # workspace_bytes 0: never launches
SIZE = Entry("wn_event_align_workspace_bytes", dict(batch=2, max_events=1000, band=64))


def test_symbols_are_exported(lib):
    ALIGN.check_exported(lib)
    SIZE.check_exported(lib)


def test_signature_rows_match_the_header():
    ALIGN.check_declared()                                           # 31 arguments
    SIZE.check_declared()                                            # 3


def test_workspace_size(lib):
    size = lib.wn_event_align_workspace_bytes
    for args in ((0, 10, 64), (-1, 10, 64), (65536, 10, 64), (1, 0, 64), (1, 2 ** 20 + 1, 64), (1, 10, 0), (1, 10, 32), (1, 10, 96),
                 (1, 10, 2112), (1, 10, -64)):
        assert size(*args) == 0, args
    assert size(65535, 1, 64) > 0 and size(1, 2 ** 20, 2048) == 2 ** 20 * 512
    for B, M, W in ((1, 1, 64), (3, 129, 576), (32, 17001, 512), (2, 1000, 64)):
        assert B * M * W // 4 <= size(B, M, W) < B * M * W // 4 + 16 and size(B, M, W) % 16 == 0       # two bits per event and slot


def test_rejects_on_the_host_in_order(lib):
    assert ALIGN(lib) == WN_ERR_WORKSPACE                            # everything else about the default call is accepted
    ALIGN.rejects(lib, "n_events",
                  shape=(dict(batch=0), dict(batch=-2), dict(max_events=0), dict(max_events=-5), dict(max_labels=0), dict(max_states=0),
                         dict(max_states=-1), dict(labels_stride=-1)),
                  unsupported=(dict(k=0), dict(k=7), dict(first=-1), dict(first=9), dict(frac_bits=-1), dict(frac_bits=21), dict(weight_shift=15),
                               dict(weight_shift=64), dict(max_cost=0), dict(max_cost=-1), dict(band=0), dict(band=32), dict(band=96),
                               dict(band=2112), dict(band=-64), dict(move_cost1=-1), dict(move_cost0=-2), dict(move_cost1=-2), dict(move_cost2=-2),
                               dict(move_cost3=-2), dict(move_cost0=2 ** 30), dict(move_cost1=2 ** 30), dict(move_cost2=2 ** 30),
                               dict(move_cost3=2 ** 30), dict(batch=65536), dict(max_events=2 ** 20 + 1), dict(max_states=2 ** 20 + 1)),
                  accepted=(dict(k=1), dict(k=6), dict(first=0), dict(first=8), dict(frac_bits=0), dict(frac_bits=20), dict(weight_shift=16),
                            dict(weight_shift=63), dict(max_cost=1), dict(max_cost=2 ** 31 - 1), dict(band=64), dict(band=128), dict(band=576),
                            dict(band=2048), dict(move_cost0=-1), dict(move_cost2=-1), dict(move_cost3=-1),
                            dict(move_cost0=-1, move_cost2=-1, move_cost3=-1), dict(move_cost0=0, move_cost1=0, move_cost2=0, move_cost3=0),
                            dict(move_cost0=2 ** 30 - 1), dict(move_cost1=2 ** 30 - 1), dict(move_cost2=2 ** 30 - 1), dict(move_cost3=2 ** 30 - 1),
                            dict(batch=65535), dict(batch=1), dict(max_events=2 ** 20), dict(max_states=2 ** 20), dict(labels_stride=0)),
                  required=("n_events", "ev_starts", "ev_sum", "ev_sumsq", "labels", "label_lengths", "model", "starts", "score", "move_counts",
                            "band_hits", "workspace"))
    for name in ("event_state", "bad"):                              # optional
        assert ALIGN(lib, **{name: None}) == WN_ERR_WORKSPACE, name
    # the workspace: too small by one byte, misaligned, and following the band
    need = SIZE(lib)
    assert need == 32000
    assert ALIGN(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert ALIGN(lib, workspace=ctypes.c_void_p((1 << 20) + 8), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert ALIGN(lib, band=128, workspace_bytes=need) == WN_ERR_WORKSPACE
    # the order: shape, then unsupported, then NULL, then workspace
    assert ALIGN(lib, batch=0, k=7, n_events=None) == WN_ERR_BAD_SHAPE
    assert ALIGN(lib, labels_stride=-1, band=96, model=None) == WN_ERR_BAD_SHAPE
    assert ALIGN(lib, max_states=0, batch=65536, workspace=None) == WN_ERR_BAD_SHAPE
    assert ALIGN(lib, k=7, ev_sum=None) == WN_ERR_UNSUPPORTED
    assert ALIGN(lib, move_cost1=-1, score=None) == WN_ERR_UNSUPPORTED
    assert ALIGN(lib, batch=65536, workspace=None) == WN_ERR_UNSUPPORTED
    assert ALIGN(lib, model=None, workspace_bytes=0) == WN_ERR_NULL


def test_move_costs_against_exact_values():
    import wavenet_speech_amd as W
    assert W.DEFAULT_MOVES == (0.14, 0.62, 0.20, 0.04)
    assert W.move_costs(W.DEFAULT_MOVES) == W.move_costs(W.DEFAULT_MOVES, 8) == (503, 122, 412, 824)
    assert W.move_costs((1.0, 1.0, 0.0, 0.0), 8) == (0, 0, -1, -1)
    assert W.move_costs((0.5, 0.25, 0.125, 0.0), 0) == (1, 1, 2, -1)                 # ln 2 = 0.69, 1.39, 2.08
    assert W.move_costs((0.5, 0.25, 0.125, 2.0 ** -40), 16) == tuple(round(n * math.log(2.0) * 65536) for n in (1, 2, 3, 40))
    assert W.move_costs((math.exp(-0.5), math.exp(-1.5), math.exp(-2.5), 1.0), 0) == (0, 2, 2, 0)       # ties to even
    assert W.move_costs([0.0, 1e-300, 0.0, 0.0], 16) == (-1, round(-math.log(1e-300) * 65536), -1, -1)
    for probs, cb in (((0.1, 0.0, 0.1, 0.1), 8), ((0.1, 0.5, 0.1), 8), ((0.1, 0.5, 0.1, 0.1, 0.1), 8), ((0.1, 0.5, -0.1, 0.1), 8),
                      ((0.1, 0.5, float("nan"), 0.1), 8), ((0.1, 0.5, float("inf"), 0.1), 8), ((0.1, 0.5, 1.5, 0.1), 8), ((0.1, 0.5, 0.1, 0.1), 17),
                      ((0.1, 0.5, 0.1, 0.1), -1), ("abcd", 8), (None, 8)):
        with pytest.raises(ValueError, match="move_costs"):
            W.move_costs(probs, cb)


def test_move_costs_of_the_defaults_digit_by_digit():
    """-ln p 256 of the four defaults: 503.33, 122.38, 412.02, 824.03"""
    import wavenet_speech_amd as W
    from tests import event_align_cases as C
    want = tuple(round(-math.log(p) * 256) for p in W.DEFAULT_MOVES)
    assert W.move_costs(W.DEFAULT_MOVES, 8) == want == C.MOVES


def test_fit_moves():
    import wavenet_speech_amd as W
    counts = torch.tensor([[10, 60, 20, 10], [-1, -1, -1, -1], [0, 0, 0, 0], [4, 64, 20, 12]], dtype=torch.int32)
    assert W.fit_moves(counts) == (14 / 200, 124 / 200, 40 / 200, 22 / 200)
    assert W.fit_moves([[0, 5, 0, 0]]) == (0.0, 1.0, 0.0, 0.0)
    again = W.move_costs(W.fit_moves(counts))
    assert again == tuple(round(-math.log(p) * 256) for p in (0.07, 0.62, 0.2, 0.11))
    for bad in ([[-1, -1, -1, -1]], [[0, 0, 0, 0]], [[3, 0, 1, 1]], [[1, 2, 3]], [1, 2, 3, 4], [[0.5, 0.5, 0.0, 0.0]]):
        with pytest.raises(ValueError, match="fit_moves"):
            W.fit_moves(bad)


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    model = W.SignalModel(torch.tensor([[10, 1 << 16, 0], [20, 1 << 16, 0], [30, 1 << 16, 0], [40, 1 << 16, 0]]), 16, frac_bits=0, cost_bits=0)
    events = (torch.tensor([1], dtype=torch.int32), torch.tensor([[0, 2, 2]], dtype=torch.int32), torch.tensor([[20, 0]]), torch.tensor([[200, 0]]))
    labels, ll = torch.ones(1, 3, dtype=torch.int32), [3]
    with pytest.raises(ValueError, match="frac_bits 12 and the model 0"):
        W.event_align(events, labels, ll, model, frac_bits=12)
    found = W.DetectedEvents(*events, torch.zeros(1, 2, dtype=torch.int32), frac_bits=12)
    with pytest.raises(ValueError, match="frac_bits 12 and the model 0"):
        W.event_align(found, labels, ll, model)
    with pytest.raises(ValueError, match="made with 12"):
        W.event_align(found, labels, ll, model, frac_bits=0)
    for kw in (dict(), dict(frac_bits=None)):                        # a tuple needs its frac_bits
        with pytest.raises(ValueError, match="with frac_bits="):
            W.event_align(events, labels, ll, model, **kw)
    with pytest.raises(ValueError, match="DetectedEvents"):
        W.event_align(events[:3], labels, ll, model, frac_bits=0)
    with pytest.raises(ValueError, match="SignalModel"):
        W.event_align(events, labels, ll, model.table, frac_bits=0)
    for kw in (dict(band=32), dict(band=96), dict(band=2112), dict(first=-1), dict(first=9), dict(max_cost=0), dict(max_cost=2 ** 31),
               dict(moves=(0.1, 0.0, 0.1, 0.1)), dict(moves=(0.1, 0.5, 0.1)), dict(moves=(5, -1, 5, 5)), dict(moves=(5, 5, -2, 5)),
               dict(moves=(5, 5, 2 ** 30, 5)), dict(moves=7)):
        with pytest.raises(ValueError, match="event_align|move_costs"):
            W.event_align(events, labels, ll, model, frac_bits=0, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.event_align(events, labels, ll, model, frac_bits=0)
