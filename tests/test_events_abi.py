"""CPU: the C ABI of the event tables (csrc/wn_events.hip): the exported symbols, the ctypes rows against the header argument by
argument, and every host-side rejection in its documented order (shape, unsupported, NULL, workspace).  The pointers are fakes:
every call below returns before anything would be launched -- none of them touches a device."""
import ctypes

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

EVENTS = Entry("wn_kmer_events", dict(signal=FAKE, signal_kind=0, signal_stride=1000, signal_lengths=FAKE, scale_shift=FAKE, seg_begin=FAKE,
                                      seg_end=FAKE, seg_row_stride=101, seg_elem_stride=1, frame_stride=1, frame_offset=0, labels=FAKE,
                                      labels_stride=100, label_lengths=FAKE, events=FAKE, batch=2, max_signal=1000, max_labels=100, max_events=100,
                                      k=5, first=-2, frac_bits=12, max_dwell=255, ev_kmer=FAKE, ev_start=FAKE, ev_len=FAKE, ev_sum=FAKE,
                                      ev_sumsq=FAKE, read_counts=FAKE, kmer_stats=FAKE, dwell_hist=FAKE, workspace=FAKE, workspace_bytes=0,
                                      bad=None, stream=None))        # workspace_bytes 0: never launches
SIZE = Entry("wn_kmer_events_workspace_bytes", dict(batch=2, max_events=100))
OUTPUTS = ("ev_kmer", "ev_start", "ev_len", "ev_sum", "ev_sumsq", "read_counts", "kmer_stats", "dwell_hist")


def test_events_symbols_are_exported(lib):
    EVENTS.check_exported(lib)
    SIZE.check_exported(lib)


def test_signature_rows_match_the_header():
    EVENTS.check_declared()                                          # 35 arguments
    SIZE.check_declared()                                            # 2


def test_workspace_size(lib):
    size = lib.wn_kmer_events_workspace_bytes
    assert size(0, 10) == 0 and size(1, 0) == 0 and size(-1, 10) == 0 and size(65536, 1) == 0
    assert size(65535, 1) > 0
    for B, N in ((1, 1), (3, 129), (32, 17000)):
        assert size(B, N) >= 20 * B + 24 * B * N and size(B, N) % 16 == 0             # flags, counts, four rows per event
        assert size(B, N) <= 20 * B + 24 * B * N + 5 * 256


def test_rejects_on_the_host_in_order(lib):
    assert EVENTS(lib) == WN_ERR_WORKSPACE                           # everything else about the default call is accepted
    EVENTS.rejects(lib, "signal",
                   shape=(dict(batch=0), dict(batch=-2), dict(max_events=0), dict(max_events=-1), dict(max_signal=0), dict(max_signal=-5),
                          dict(max_labels=0), dict(signal_stride=-1), dict(seg_row_stride=-1), dict(seg_elem_stride=-2), dict(labels_stride=-1),
                          dict(frame_stride=0), dict(frame_stride=-3), dict(frame_offset=-1), dict(signal_kind=2), dict(signal_kind=-1)),
                   unsupported=(dict(k=0), dict(k=7), dict(first=9), dict(first=-9), dict(frac_bits=-1), dict(frac_bits=21), dict(max_dwell=0),
                                dict(max_dwell=65537), dict(batch=65536), dict(max_signal=2 ** 31 - 1, frame_stride=2),
                                dict(max_signal=2 ** 30, frame_stride=2), dict(max_signal=1000, frame_stride=2 ** 31 // 1000 + 1)),
                   accepted=(dict(k=1), dict(k=6), dict(first=8), dict(first=-8), dict(frac_bits=0), dict(frac_bits=20), dict(max_dwell=1),
                             dict(max_dwell=65536), dict(batch=65535), dict(batch=1), dict(max_signal=2 ** 31 - 1),
                             dict(max_signal=2 ** 30 - 1, frame_stride=2), dict(signal_kind=1), dict(frame_offset=7),
                             dict(signal_stride=0, seg_row_stride=0, seg_elem_stride=0, labels_stride=0)),
                   required=("signal", "signal_lengths", "seg_begin", "seg_end", "labels", "label_lengths", "events"))
    assert EVENTS(lib, scale_shift=None) == WN_ERR_WORKSPACE         # optional
    assert EVENTS(lib, workspace=None) == WN_ERR_NULL                # tables without a workspace
    assert EVENTS(lib, workspace=None, kmer_stats=None, dwell_hist=None) == WN_ERR_NULL     # the per-read flags live there too
    nothing = {name: None for name in OUTPUTS}
    assert EVENTS(lib, **nothing) == WN_ERR_NULL                     # nothing to compute
    assert EVENTS(lib, bad=FAKE, **nothing) == WN_ERR_NULL           # the counter is no output
    for name in OUTPUTS:                                             # any one output is enough
        assert EVENTS(lib, **dict(nothing, **{name: FAKE})) == WN_ERR_WORKSPACE, name
    # the workspace: too small by one byte, misaligned, and a signal off its element size
    need = SIZE(lib)
    assert EVENTS(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert EVENTS(lib, workspace=ctypes.c_void_p((1 << 20) + 8), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert EVENTS(lib, signal=ctypes.c_void_p((1 << 20) + 2), workspace_bytes=need) == WN_ERR_WORKSPACE
    assert EVENTS(lib, signal=ctypes.c_void_p((1 << 20) + 1), signal_kind=1, workspace_bytes=need) == WN_ERR_WORKSPACE
    # the order: shape, then unsupported, then NULL, then workspace
    assert EVENTS(lib, batch=0, k=7, signal=None) == WN_ERR_BAD_SHAPE
    assert EVENTS(lib, signal_kind=2, max_dwell=0, **nothing) == WN_ERR_BAD_SHAPE
    assert EVENTS(lib, frame_stride=0, batch=65536, workspace=None) == WN_ERR_BAD_SHAPE
    assert EVENTS(lib, k=7, signal=None) == WN_ERR_UNSUPPORTED
    assert EVENTS(lib, first=9, **nothing) == WN_ERR_UNSUPPORTED
    assert EVENTS(lib, batch=65536, workspace=None) == WN_ERR_UNSUPPORTED
    assert EVENTS(lib, events=None, workspace_bytes=0) == WN_ERR_NULL
