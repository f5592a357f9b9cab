"""CPU: the C ABI of the event detection (csrc/wn_eventdetect.hip): the exported symbols, the ctypes rows against the header argument
by argument, the size function on both sides of its limits, and every host-side rejection on both sides of its limit and in its
documented order (shape, unsupported, NULL, workspace), with fake pointers: every call below returns before anything would be
launched.  And what detect_events refuses before it reaches the library."""
import ctypes

import pytest
import torch

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

DETECT = Entry("wn_event_detect", dict(signal=FAKE, signal_kind=0, signal_stride=1000, signal_lengths=FAKE, scale_shift=FAKE, batch=2, max_signal=1000,
                                       frac_bits=12, window_short=3, window_long=6, radius_short=3, radius_long=6, threshold_short=4096,
                                       threshold_long=9216, min_var_short=100, min_var_long=400, max_event_len=65536, max_events=1000,
                                       chunk_samples=0, n_events=FAKE, starts=FAKE, ev_sum=FAKE, ev_sumsq=FAKE, ev_kind=FAKE, workspace=FAKE,
                                       workspace_bytes=0, bad=None, stream=None))    # workspace_bytes 0: never launches
SIZE = Entry("wn_event_detect_workspace_bytes", dict(batch=2, max_signal=1000))


def test_symbols_are_exported(lib):
    DETECT.check_exported(lib)
    SIZE.check_exported(lib)


def test_signature_rows_match_the_header():
    DETECT.check_declared()                                          # 28 arguments
    SIZE.check_declared()                                            # 2


def test_size_function(lib):
    size = lib.wn_event_detect_workspace_bytes
    for args in ((0, 100), (-1, 100), (65536, 100), (1, 0), (1, -5), (1, 2 ** 24 + 1)):
        assert size(*args) == 0, args
    for B, L in ((1, 1), (3, 64), (3, 65), (65535, 1000), (4, 2 ** 24), (256, 2 ** 18)):
        need = 4 * B + 2 * 8 * B * ((L + 63) // 64)                  # a flag per read and two bits per sample, in 64-bit words
        assert need <= size(B, L) < need + 3 * 256 and size(B, L) % 16 == 0, (B, L)


def test_rejects_on_the_host_in_order(lib):
    assert DETECT(lib) == WN_ERR_WORKSPACE                           # everything else about the default call is accepted
    DETECT.rejects(lib, "signal",
                   shape=(dict(batch=0), dict(batch=-2), dict(max_signal=0), dict(max_signal=-5), dict(max_events=0), dict(max_events=-1),
                          dict(signal_stride=-1), dict(signal_kind=2), dict(signal_kind=-1)),
                   unsupported=(dict(frac_bits=-1), dict(frac_bits=21), dict(batch=65536), dict(max_signal=2 ** 24 + 1), dict(max_events=2 ** 24 + 1),
                                dict(window_short=0), dict(window_short=17), dict(window_long=-1), dict(window_long=17), dict(radius_short=0),
                                dict(radius_short=65), dict(radius_long=0), dict(radius_long=65), dict(threshold_short=0), dict(threshold_long=0),
                                dict(threshold_long=-7), dict(min_var_short=0), dict(min_var_short=2 ** 55 + 1), dict(min_var_long=0),
                                dict(min_var_long=2 ** 55 + 1), dict(max_event_len=0), dict(max_event_len=65537), dict(chunk_samples=128),
                                dict(chunk_samples=-256), dict(chunk_samples=384), dict(chunk_samples=16384 + 256), dict(chunk_samples=1)),
                   accepted=(dict(frac_bits=0), dict(frac_bits=20), dict(batch=65535), dict(batch=1), dict(max_signal=2 ** 24), dict(max_signal=1),
                             dict(max_events=2 ** 24), dict(max_events=1), dict(window_short=1), dict(window_short=16), dict(window_long=0),
                             dict(window_long=16), dict(radius_short=1), dict(radius_short=64), dict(radius_long=1), dict(radius_long=64),
                             dict(threshold_short=1), dict(threshold_long=2 ** 31 - 1), dict(min_var_short=1), dict(min_var_short=2 ** 55),
                             dict(min_var_long=1), dict(min_var_long=2 ** 55), dict(max_event_len=1), dict(max_event_len=65536),
                             dict(chunk_samples=256), dict(chunk_samples=768), dict(chunk_samples=16384), dict(signal_kind=1), dict(signal_stride=0),
                             dict(window_long=0, radius_long=0, threshold_long=0, min_var_long=0)),   # the long detector off: its three are ignored
                   required=("signal", "signal_lengths", "n_events", "starts", "ev_sum", "ev_sumsq", "workspace"))
    for name in ("scale_shift", "ev_kind", "bad"):                   # optional
        assert DETECT(lib, **{name: None}) == WN_ERR_WORKSPACE, name
    # the workspace: too small by one byte, misaligned, and a signal off its element size
    need = SIZE(lib)
    assert DETECT(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert DETECT(lib, workspace=ctypes.c_void_p((1 << 20) + 8), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert DETECT(lib, signal=ctypes.c_void_p((1 << 20) + 2), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert DETECT(lib, signal=ctypes.c_void_p((1 << 20) + 1), signal_kind=1, workspace_bytes=need) == WN_ERR_WORKSPACE
    assert DETECT(lib, batch=300, workspace_bytes=need) == WN_ERR_WORKSPACE          # the size follows the batch
    # the order: shape, then unsupported, then NULL, then workspace
    assert DETECT(lib, batch=0, frac_bits=21, signal=None) == WN_ERR_BAD_SHAPE
    assert DETECT(lib, signal_kind=2, chunk_samples=100, starts=None) == WN_ERR_BAD_SHAPE
    assert DETECT(lib, max_events=0, batch=65536, workspace=None) == WN_ERR_BAD_SHAPE
    assert DETECT(lib, window_short=17, signal=None) == WN_ERR_UNSUPPORTED
    assert DETECT(lib, max_event_len=0, n_events=None) == WN_ERR_UNSUPPORTED
    assert DETECT(lib, chunk_samples=100, workspace=None) == WN_ERR_UNSUPPORTED
    assert DETECT(lib, ev_sum=None, workspace_bytes=0) == WN_ERR_NULL


def test_python_surface_refusals():
    import wavenet_speech_amd as W
    from wavenet_speech_amd import events
    assert W.detect_events is events.detect_events and W.DetectedEvents is events.DetectedEvents
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # the signal is looked at first, as in the other read tools
        W.detect_events(torch.zeros(1, 10), [10])
    assert len(events.DEFAULT_THRESHOLDS) == 2 and events.DEFAULT_MIN_VAR > 0
    assert (events.MAX_DETECT_WINDOW, events.MAX_DETECT_RADIUS, events.MAX_DETECT_VMIN, events.MAX_EVENT_LEN) == (16, 64, 2 ** 55, 65536)
    # the two places that turn detect_events' floats into the integers of the C ABI agree
    from tests import event_detect_ref as R
    assert R.theta_of(4.0) == 4096 and R.theta_of(1e-9) == 1 and R.vmin_of(0.0, 12, 3) == 1 and R.vmin_of(0.01, 12, 6) == 6039798
