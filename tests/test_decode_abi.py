"""CPU: the C ABI of the CTC decoders (csrc/wn_decode.hip): exported symbols, the ctypes rows against the header, workspace sizes,
and the shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls below touches a device."""
import ctypes

from tests.abi_util import FAKE, WN_ERR_NULL, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

X = dict(x=FAKE, sb=lambda a: a["classes"] * a["length"], sc=lambda a: a["length"], st=1)           # [B][C][T], dense
GREEDY = Entry("wn_ctc_greedy_decode", dict(X, input_lengths=None, batch=2, classes=5, length=10, blank=0, labels=FAKE, frames=None, lengths=FAKE,
                                            bad=None, stream=None))
BEAM = Entry("wn_ctc_beam_decode", dict(X, input_kind=0, input_lengths=None, batch=2, classes=5, length=10, blank=0, beam_width=4, labels=FAKE,
                                        frames=None, lengths=FAKE, scores=FAKE, workspace=FAKE, workspace_bytes=1 << 30, bad=None, stream=None))
SIZE = Entry("wn_ctc_decode_workspace_bytes", dict(batch=2, classes=5, length=10, beam_width=4))


def test_decode_symbols_are_exported(lib):
    for entry in (SIZE, GREEDY, BEAM):                               # 4, 14 and 19 arguments
        entry.check_exported(lib)
        entry.check_declared()


def test_workspace_bytes(lib):
    for B, C, T, W in [(1, 2, 1, 1), (8, 5, 1000, 8), (32, 5, 4096, 64), (2, 64, 100, 64)]:
        n = lib.wn_ctc_decode_workspace_bytes(B, C, T, W)
        assert n >= B * T * W * 8 and n % 16 == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 5, 1000, 0) == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 5, 1000, 65) == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 65, 1000, 8) == 0
    assert lib.wn_ctc_decode_workspace_bytes(0, 5, 1000, 8) == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 1, 1000, 8) == 0
    assert lib.wn_ctc_decode_workspace_bytes(8, 5, 0, 8) == 0


def test_beam_decode_rejects_on_the_host(lib):
    BEAM.rejects(lib, "x", shape=(dict(beam_width=0), dict(batch=0), dict(classes=1), dict(length=0), dict(input_kind=3)),
                 unsupported=(dict(classes=65), dict(beam_width=65)), required=("workspace",))
    assert BEAM(lib, x=None, labels=None, lengths=None, scores=None) == WN_ERR_NULL
    assert BEAM(lib, workspace_bytes=16) == WN_ERR_WORKSPACE
    assert BEAM(lib, workspace=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE       # not 16-byte aligned


def test_greedy_decode_rejects_on_the_host(lib):
    GREEDY.rejects(lib, "x", shape=(dict(classes=1), dict(batch=0), dict(length=0)), unsupported=(dict(classes=65),))
    assert GREEDY(lib, x=None, labels=None, lengths=None) == WN_ERR_NULL
