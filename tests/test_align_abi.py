"""CPU: the C ABI of CTC forced alignment (csrc/wn_align.hip): exported symbols, the ctypes rows against the header, workspace
sizes, and the shape / limit / pointer checks, which run on the host before any HIP call -- none of the calls below touches a
device."""
import ctypes

from tests.abi_util import FAKE, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

ALIGN = Entry("wn_ctc_align", dict(x=FAKE, sb=lambda a: a["classes"] * a["length"], sc=lambda a: a["length"], st=1, input_kind=0, labels=FAKE,
                                   label_lengths=FAKE, input_lengths=None, batch=2, classes=5, length=10, max_label_len=4, blank=0, states=FAKE,
                                   frame_labels=None, spans=None, score=FAKE, workspace=FAKE, workspace_bytes=1 << 30, bad=None, stream=None))
SIZE = Entry("wn_ctc_align_workspace_bytes", dict(batch=2, classes=5, length=10, max_label_len=4))


def test_align_symbols_are_exported(lib):
    for entry in (ALIGN, SIZE):                                      # 21 and 4 arguments
        entry.check_exported(lib)
        entry.check_declared()


def test_workspace_bytes(lib):
    for B, C, T, L in [(1, 2, 1, 1), (8, 5, 1000, 100), (32, 5, 4096, 410), (8, 5, 4096, 2047), (2, 64, 100, 31), (3, 5, 77, 32)]:
        n = lib.wn_ctc_align_workspace_bytes(B, C, T, L)
        sp = (2 * L + 1 + 63) // 64 * 64
        assert n % 16 == 0
        assert n >= B * T * ((2 * L + 1 + 3) // 4)                   # 2 bits per state and frame
        assert n <= B * T * (sp + 16) + 256                          # the loss takes 16 bytes per state and frame
        assert n <= lib.wn_ctc_workspace_bytes(B, C, T, L) // 16
    for B, C, T, L in [(0, 5, 100, 10), (8, 1, 100, 10), (8, 5, 0, 10), (8, 5, 100, 0), (-1, 5, 100, 10), (8, 5, 100, -3),
                       (8, 65, 100, 10), (8, 5, 100, 2048), (8, 5, (1 << 24) + 1, 10), (65536, 5, 100, 10),
                       (65535, 5, 1 << 16, 10)]:
        assert lib.wn_ctc_align_workspace_bytes(B, C, T, L) == 0, (B, C, T, L)


def test_align_rejects_on_the_host(lib):
    ALIGN.rejects(lib, "x",
                  shape=(dict(batch=0), dict(classes=1), dict(length=0), dict(max_label_len=0), dict(input_kind=3), dict(input_kind=-1),
                         dict(blank=5), dict(blank=-1)),
                  unsupported=(dict(classes=65), dict(max_label_len=2048), dict(length=(1 << 24) + 1), dict(batch=65536)),
                  required=("x", "labels", "label_lengths", "states", "score", "workspace"))
    need = SIZE(lib)
    assert need > 0
    assert ALIGN(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert ALIGN(lib, workspace_bytes=0) == WN_ERR_WORKSPACE
    assert ALIGN(lib, workspace=ctypes.c_void_p((1 << 20) + 8)) == WN_ERR_WORKSPACE      # not 16-byte aligned
    # the order of the checks: shape, then unsupported, then NULL, then workspace
    assert ALIGN(lib, batch=0, classes=65, x=None) == WN_ERR_BAD_SHAPE
    assert ALIGN(lib, classes=65, x=None, workspace_bytes=0) == WN_ERR_UNSUPPORTED
    assert ALIGN(lib, x=None, workspace_bytes=0) == WN_ERR_NULL
