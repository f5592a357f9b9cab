"""The drivers of the signal tools on the device (kmer_events, detect_events, event_align, signal_align, signal_map):
a case of tests/*_cases.py through the tool, and the exact comparison of each result class with the reference's dict.  Used by
the tools' own files, tests/test_gpu_signal_limits.py, test_gpu_tool_limits.py and test_gpu_wave_steps.py.  Everything these
kernels write is an integer and every comparison exact equality; nothing here is rewritten by pytest, so every assert carries its
message."""
import numpy as np
import torch

import wavenet_speech_amd as W
from tests import event_align_cases as EA
from tests import event_align_ref as EAR
from tests import event_detect_cases as ED
from tests import kmer_events_cases as EC
from tests import signal_align_cases as SC
from tests.gpu_util import assert_equal_arrays, dev, i64
from tests.gpu_util import strided as strided_view

EVENT_FIELDS = ("kmer", "start", "length", "sum", "sumsq")


def _field(got, name, dtype, want):
    """one tensor of a result: its dtype, then shape and every element"""
    t = getattr(got, name)
    assert t.dtype == dtype, "%s is %s, expected %s" % (name, t.dtype, dtype)
    assert_equal_arrays(t.cpu().numpy(), want, name)


def model_of(case):
    """the integer model of a signal_align / signal_map case as a hand-filled SignalModel"""
    table = torch.from_numpy(case.model)
    model = W.SignalModel(table.clamp(min=1) if bool((table[:, 1] < 1).any()) else table, case.kw["weight_shift"], case.kw["frac_bits"],
                          SC.COST_BITS)
    model.table.copy_(table)                                         # the constructor refuses a weight of 0: the device must too
    return model


# ---- kmer_events --------------------------------------------------------------------------------------------------------------------

def kmer_events(case, layout, kind, frac_bits, seg=None, strided=False, **more):
    if kind == "f32":
        signal, ss = case.signal, None
    else:
        signal, ss = more.pop("int16")
    signal = strided_view(signal, kind == "f32") if strided else dev(signal)
    if seg is None:
        seg = EC.spans_of(case) if layout == "spans" else case.starts
    kw = dict(dict(max_dwell=255), **case.kw)
    kw.update(more)
    return W.kmer_events(signal, dev(case.signal_lengths), dev(case.labels), dev(case.label_lengths), frac_bits=frac_bits,
                         scale_shift=None if ss is None else dev(ss), **{layout: dev(seg)}, **kw)


def assert_kmer_events(got, ref, events=True):
    if events:
        for name in EVENT_FIELDS:
            _field(got, name, torch.int64 if name in ("sum", "sumsq") else torch.int32, ref[name])
    else:
        assert all(f is None for f in got[:5]), "event fields were returned: %s" % [f is not None for f in got[:5]]
    _field(got, "read_counts", torch.int32, ref["read_counts"])
    _field(got, "kmer_stats", torch.int64, ref["kmer_stats"])
    _field(got, "dwell_hist", torch.int64, ref["dwell_hist"])


# ---- detect_events ------------------------------------------------------------------------------------------------------------------

def detect_events(case, signal=None, scale_shift=None, chunk=ED.CHUNK, **more):
    signal = dev(case.signal) if signal is None else signal
    kw = dict(case.kw, **more)
    return W.detect_events(signal, dev(case.signal_lengths), scale_shift=None if scale_shift is None else dev(scale_shift), chunk=chunk, **kw)


def assert_detected(got, ref):
    for name in ("n_events", "starts", "kind"):
        _field(got, name, torch.int32, ref[name])
    for name in ("sum", "sumsq"):
        _field(got, name, torch.int64, i64(ref[name]))


# ---- event_align --------------------------------------------------------------------------------------------------------------------

def event_model(case):
    return W.SignalModel(torch.from_numpy(case.model), case.kw["weight_shift"], frac_bits=EA.F, cost_bits=EA.COST_BITS)


def event_tables(case):
    """the events of a case as the tuple event_align takes"""
    return (dev(case.n_events), dev(case.ev_starts), dev(case.ev_sum), dev(case.ev_sumsq))


def event_align(case, band=None, states=True, labels=None, model=None, moves=None):
    kw = case.kw
    return W.event_align(event_tables(case), dev(case.labels) if labels is None else labels, dev(case.label_lengths),
                         event_model(case) if model is None else model, first=kw["first"], band=kw["band"] if band is None else band,
                         moves=kw["move_cost"] if moves is None else moves, max_cost=kw["max_cost"], want_states=states, frac_bits=EA.F)


def assert_event_alignment(got, ref, states=True):
    assert got.score.dtype == torch.int64, "score is %s" % got.score.dtype
    assert got.score.tolist() == [int(v) for v in ref["score"]], "score: %s, expected %s" % (got.score.tolist(), [int(v) for v in ref["score"]])
    for name in ("starts", "band_hits", "moves"):
        _field(got, name, torch.int32, ref[name])
    if states:
        _field(got, "states", torch.int32, ref["states"])
    else:
        assert got.states is None, "states were returned"


def assert_move_counts(got, case, ref):
    """1 + sum counts = E and counts[1] + 2 counts[2] + 3 counts[3] = N - 1 on every aligned read"""
    kw = case.kw
    moves = got.moves.cpu().numpy().astype(np.int64)
    for b, sc in enumerate(ref["score"]):
        if sc in (EAR.NO_ALIGNMENT, EAR.BAD_READ):
            continue
        N = int(case.label_lengths[b]) - (kw["k"] - 1) - 2 * kw["first"]
        assert 1 + moves[b].sum() == case.n_events[b] and moves[b, 1] + 2 * moves[b, 2] + 3 * moves[b, 3] == N - 1, \
            "read %d: moves %s for %d events and %d states" % (b, moves[b].tolist(), case.n_events[b], N)


# ---- signal_align and signal_map ----------------------------------------------------------------------------------------------------

def assert_signal_alignment(got, ref, states=True):
    _field(got, "starts", torch.int32, ref["starts"])
    assert got.score.dtype == torch.int64, "score is %s" % got.score.dtype
    assert got.score.cpu().tolist() == ref["score"].tolist(), "score: %s, expected %s" % (got.score.cpu().tolist(), ref["score"].tolist())
    _field(got, "band_hits", torch.int32, ref["band_hits"])
    if states:
        _field(got, "states", torch.int32, ref["states"])
    else:
        assert got.states is None, "states were returned"


def assert_signal_mapping(got, ref, end_cost=True):
    for name in ("score", "runner_up", "block_cost"):
        _field(got, name, torch.int64, i64(ref[name]))
    for name in ("end", "start", "block_end"):
        _field(got, name, torch.int32, ref[name])
    if end_cost:
        _field(got, "end_cost", torch.int64, i64(ref["end_cost"]))
    else:
        assert got.end_cost is None, "end_cost was returned"
