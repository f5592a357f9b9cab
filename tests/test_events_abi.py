"""CPU: the C ABI of the event tables (csrc/wn_events.hip): the exported symbols, the ctypes rows against the header argument by
argument, and every host-side rejection in its documented order (shape, unsupported, NULL, workspace).  The pointers are fakes:
every call below returns before anything would be launched -- none of them touches a device."""
import ctypes

import pytest

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, check_row, header_names

NAME = "wn_kmer_events"
ARGS = ["signal", "signal_kind", "signal_stride", "signal_lengths", "scale_shift", "seg_begin", "seg_end", "seg_row_stride",
        "seg_elem_stride", "frame_stride", "frame_offset", "labels", "labels_stride", "label_lengths", "events", "batch", "max_signal",
        "max_labels", "max_events", "k", "first", "frac_bits", "max_dwell", "ev_kmer", "ev_start", "ev_len", "ev_sum", "ev_sumsq",
        "read_counts", "kmer_stats", "dwell_hist", "workspace", "workspace_bytes", "bad", "stream"]
INPUTS = ("signal", "signal_lengths", "seg_begin", "seg_end", "labels", "label_lengths", "events")
OUTPUTS = ("ev_kmer", "ev_start", "ev_len", "ev_sum", "ev_sumsq", "read_counts", "kmer_stats", "dwell_hist")


@pytest.fixture(scope="module")
def lib():
    from wavenet_speech_amd import _lib
    return _lib.load()


def test_events_symbols_are_exported(lib):
    from wavenet_speech_amd import _lib
    for name in (NAME, NAME + "_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.wn_version() == 300                                   # an additive entry point


def test_signature_rows_match_the_header():
    for name, count in ((NAME, 35), (NAME + "_workspace_bytes", 2)):
        check_row(name, count=count, opaque=True)
    names = header_names(NAME)
    assert names == ARGS


def _call(lib, **kw):
    a = dict(signal=FAKE, signal_kind=0, signal_stride=1000, signal_lengths=FAKE, scale_shift=FAKE, seg_begin=FAKE, seg_end=FAKE,
             seg_row_stride=101, seg_elem_stride=1, frame_stride=1, frame_offset=0, labels=FAKE, labels_stride=100, label_lengths=FAKE,
             events=FAKE, batch=2, max_signal=1000, max_labels=100, max_events=100, k=5, first=-2, frac_bits=12, max_dwell=255,
             ev_kmer=FAKE, ev_start=FAKE, ev_len=FAKE, ev_sum=FAKE, ev_sumsq=FAKE, read_counts=FAKE, kmer_stats=FAKE,
             dwell_hist=FAKE, workspace=FAKE, workspace_bytes=0, bad=None, stream=None)       # workspace_bytes 0: never launches
    assert set(kw) <= set(a), kw
    a.update(kw)
    return lib.wn_kmer_events(*[a[n] for n in ARGS])


def test_workspace_size(lib):
    size = lib.wn_kmer_events_workspace_bytes
    assert size(0, 10) == 0 and size(1, 0) == 0 and size(-1, 10) == 0 and size(65536, 1) == 0
    assert size(65535, 1) > 0
    for B, N in ((1, 1), (3, 129), (32, 17000)):
        assert size(B, N) >= 20 * B + 24 * B * N and size(B, N) % 16 == 0             # flags, counts, four rows per event
        assert size(B, N) <= 20 * B + 24 * B * N + 5 * 256


def test_rejects_on_the_host_in_order(lib):
    assert _call(lib) == WN_ERR_WORKSPACE                            # everything else about the default call is accepted
    for kw in (dict(batch=0), dict(batch=-2), dict(max_events=0), dict(max_events=-1), dict(max_signal=0), dict(max_signal=-5),
               dict(max_labels=0), dict(signal_stride=-1), dict(seg_row_stride=-1), dict(seg_elem_stride=-2), dict(labels_stride=-1),
               dict(frame_stride=0), dict(frame_stride=-3), dict(frame_offset=-1), dict(signal_kind=2), dict(signal_kind=-1)):
        assert _call(lib, **kw) == WN_ERR_BAD_SHAPE, kw
    for kw in (dict(k=0), dict(k=7), dict(first=9), dict(first=-9), dict(frac_bits=-1), dict(frac_bits=21), dict(max_dwell=0),
               dict(max_dwell=65537), dict(batch=65536), dict(max_signal=2 ** 31 - 1, frame_stride=2),
               dict(max_signal=2 ** 30, frame_stride=2), dict(max_signal=1000, frame_stride=2 ** 31 // 1000 + 1)):
        assert _call(lib, **kw) == WN_ERR_UNSUPPORTED, kw
    # the accepted side of each limit goes on to the pointer checks
    for kw in (dict(k=1), dict(k=6), dict(first=8), dict(first=-8), dict(frac_bits=0), dict(frac_bits=20), dict(max_dwell=1),
               dict(max_dwell=65536), dict(batch=65535), dict(batch=1), dict(max_signal=2 ** 31 - 1), dict(max_signal=2 ** 30 - 1, frame_stride=2),
               dict(signal_kind=1), dict(frame_offset=7), dict(signal_stride=0, seg_row_stride=0, seg_elem_stride=0, labels_stride=0)):
        assert _call(lib, signal=None, **kw) == WN_ERR_NULL, kw
    for name in INPUTS:
        assert _call(lib, **{name: None}) == WN_ERR_NULL, name
    assert _call(lib, scale_shift=None) == WN_ERR_WORKSPACE          # optional
    assert _call(lib, workspace=None) == WN_ERR_NULL                 # tables without a workspace
    assert _call(lib, workspace=None, kmer_stats=None, dwell_hist=None) == WN_ERR_NULL      # the per-read flags live there too
    nothing = {name: None for name in OUTPUTS}
    assert _call(lib, **nothing) == WN_ERR_NULL                      # nothing to compute
    assert _call(lib, bad=FAKE, **nothing) == WN_ERR_NULL            # the counter is no output
    for name in OUTPUTS:                                             # any one output is enough
        assert _call(lib, **dict(nothing, **{name: FAKE})) == WN_ERR_WORKSPACE, name
    # the workspace: too small by one byte, misaligned, and a signal off its element size
    need = lib.wn_kmer_events_workspace_bytes(2, 100)
    assert _call(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert _call(lib, workspace=ctypes.c_void_p((1 << 20) + 8), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert _call(lib, signal=ctypes.c_void_p((1 << 20) + 2), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert _call(lib, signal=ctypes.c_void_p((1 << 20) + 1), signal_kind=1, workspace_bytes=need) == WN_ERR_WORKSPACE
    # the order: shape, then unsupported, then NULL, then workspace
    assert _call(lib, batch=0, k=7, signal=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, signal_kind=2, max_dwell=0, **nothing) == WN_ERR_BAD_SHAPE
    assert _call(lib, frame_stride=0, batch=65536, workspace=None) == WN_ERR_BAD_SHAPE
    assert _call(lib, k=7, signal=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, first=9, **nothing) == WN_ERR_UNSUPPORTED
    assert _call(lib, batch=65536, workspace=None) == WN_ERR_UNSUPPORTED
    assert _call(lib, events=None, workspace_bytes=0) == WN_ERR_NULL
