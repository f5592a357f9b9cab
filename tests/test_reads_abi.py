"""CPU: the C ABI of the ragged read generator (csrc/wn_reads.hip): exported symbols, the ctypes table against the header, the
workspace formula, and the shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls
below touches a device."""
import ctypes
import re

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry, header_text
from tests.abi_util import lib  # noqa: F401

FIXED, UNIFORM, GAMMA = 0, 1, 2
SIZE = Entry("wn_reads_workspace_bytes", dict(batch=2, max_bases=30))
PLAN = Entry("wn_reads_plan", dict(seed=1, batch=2, min_bases=20, max_bases=30, window=2, dwell_model=UNIFORM, dwell_p0=6.0, dwell_p1=2.0,
                                   dwell_p2=0.0, max_dwell=7, base_lengths_in=None, bases_in=None, dwell_in=None, base_lengths=FAKE, bases=FAKE,
                                   dwell=FAKE, starts=FAKE, signal_lengths=FAKE, workspace=FAKE, workspace_bytes=1 << 40, bad=None, clamped=None,
                                   stream=None))
SIGNAL = Entry("wn_reads_signal", dict(base_lengths=FAKE, starts=FAKE, signal_lengths=FAKE, workspace=FAKE, workspace_bytes=1 << 40, batch=2,
                                       max_bases=30, window=2, ld=100, means=FAKE, stdvs=FAKE, seed=1, noise=None, signal=FAKE, sample_kmer=None,
                                       clipped_lengths=None, bad=None, stream=None))


def _dwell(model, p0, p1, p2):
    return dict(dwell_model=model, dwell_p0=p0, dwell_p1=p1, dwell_p2=p2)


def test_reads_symbols_are_exported(lib):
    for entry in (SIZE, PLAN, SIGNAL):
        entry.check_exported(lib)


def test_signature_table_matches_the_header():
    for entry in (SIZE, PLAN, SIGNAL):                               # 2, 23 and 18 arguments
        entry.check_declared()
    assert re.search(r"WN_DWELL_FIXED = 0, WN_DWELL_UNIFORM = 1, WN_DWELL_GAMMA = 2", header_text())


def test_workspace_bytes(lib):
    for B, n in [(1, 1), (1, 10), (32, 701), (16, 2700), (3, 8), (3, 9), (65535, 30), (2, 65536)]:
        got = lib.wn_reads_workspace_bytes(B, n)
        assert got == B * ((n + 7) // 8 * 8) * 2, (B, n)             # one 16-bit 5-mer index per k-mer, rows of a multiple of 8
        assert got % 16 == 0 and got >= B * (n - 4) * 2
    for B, n in [(0, 10), (-1, 10), (4, 0), (4, -2), (65536, 10), (4, 65537)]:
        assert lib.wn_reads_workspace_bytes(B, n) == 0, (B, n)


def test_reads_plan_rejects_on_the_host(lib):
    PLAN.rejects(lib, "base_lengths",
                 # shapes and parameters
                 shape=(dict(batch=0), dict(batch=-2), dict(max_bases=0), dict(max_dwell=0), dict(window=1), dict(window=-2), dict(window=3),
                        dict(min_bases=8), dict(min_bases=4, window=0), dict(min_bases=30), dict(min_bases=31), dict(dwell_model=3),
                        dict(dwell_model=-1), _dwell(FIXED, 0.0, 0.0, 0.0), _dwell(UNIFORM, 0.0, 2.0, 0.0), _dwell(UNIFORM, 1.0, 0.0, 0.0),
                        _dwell(UNIFORM, 6.0, -1.0, 0.0), _dwell(UNIFORM, 6.0, 0.0, 0.0), _dwell(GAMMA, 0.0, 1.0, 1.0), _dwell(GAMMA, 1.0, 0.0, 1.0),
                        _dwell(GAMMA, 1.0, 1.0, -4.0), _dwell(GAMMA, float("nan"), 1.0, 1.0), _dwell(GAMMA, 1.0, float("inf"), 1.0)),
                 # every limit: WN_ERR_UNSUPPORTED
                 unsupported=(dict(batch=65536), dict(max_bases=65537),
                              dict(max_bases=1005, max_dwell=2147484)),                        # 1000 * 2147484 = 2^31 + 352
                 # the accepted side of each edge goes on to the pointer checks
                 accepted=(dict(batch=65535), dict(max_bases=65536),
                           dict(max_bases=1005, max_dwell=2147483),                            # 1000 * 2147483 = 2^31 - 648
                           dict(min_bases=9), dict(min_bases=5, window=0), dict(min_bases=29),
                           _dwell(UNIFORM, 1.0, 1.0, 0.0),                                     # [1, 2)
                           _dwell(GAMMA, 0.5, 587.0, 4000.0)),
                 # required pointers; the three *_in, bad and clamped are optional (they are NULL in every call here)
                 required=("base_lengths", "bases", "dwell", "starts", "signal_lengths", "workspace"))
    need = SIZE(lib)
    assert need == 2 * 32 * 2
    assert PLAN(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert PLAN(lib, workspace_bytes=0) == WN_ERR_WORKSPACE
    assert PLAN(lib, workspace=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE       # not 16-byte aligned
    # the order of the checks: shape, then unsupported, then NULL, then workspace
    assert PLAN(lib, batch=0, max_bases=65537, bases=None) == WN_ERR_BAD_SHAPE
    assert PLAN(lib, window=1, batch=65536, bases=None) == WN_ERR_BAD_SHAPE
    assert PLAN(lib, batch=65536, bases=None, workspace_bytes=0) == WN_ERR_UNSUPPORTED
    assert PLAN(lib, bases=None, workspace_bytes=0) == WN_ERR_NULL


def test_limit_edge_of_the_signal_length(lib):
    # (max_bases - 5) * max_dwell < 2^31 exactly: 65531 * 32771 = 2147516401 >= 2^31 > 65531 * 32770 = 2147450870
    assert 65531 * 32770 < 2 ** 31 <= 65531 * 32771
    assert PLAN(lib, max_bases=65536, max_dwell=32771) == WN_ERR_UNSUPPORTED
    assert PLAN(lib, max_bases=65536, max_dwell=32770, base_lengths=None) == WN_ERR_NULL


def test_reads_signal_rejects_on_the_host(lib):
    SIGNAL.rejects(lib, "signal", shape=(dict(batch=0), dict(max_bases=0), dict(ld=0), dict(ld=-5), dict(window=1), dict(window=4)),
                   unsupported=(dict(batch=65536), dict(max_bases=65537), dict(ld=2 ** 31 - 256)), accepted=(dict(ld=2 ** 31 - 257),),
                   required=("base_lengths", "starts", "signal_lengths", "workspace", "means", "stdvs", "signal"))
    need = SIZE(lib)
    assert SIGNAL(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert SIGNAL(lib, workspace=ctypes.c_void_p((1 << 20) + 4)) == WN_ERR_WORKSPACE
    assert SIGNAL(lib, ld=0, batch=65536, signal=None) == WN_ERR_BAD_SHAPE
    assert SIGNAL(lib, batch=65536, signal=None, workspace_bytes=0) == WN_ERR_UNSUPPORTED
    assert SIGNAL(lib, signal=None, workspace_bytes=0) == WN_ERR_NULL
