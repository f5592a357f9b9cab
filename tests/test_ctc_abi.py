"""CPU: the C ABI of the CTC loss (csrc/wn_ctc.hip): exported symbols, the ctypes rows against the header, the workspace size, and
the shape / limit / pointer / workspace checks, which run on the host before any HIP call -- none of the calls below touches a
device."""
import ctypes
import os
import re

from tests.abi_util import FAKE, ROOT, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

MAX_CLASSES, MAX_LABELS, MAX_BATCH = 64, 2047, 65535
LOSS = Entry("wn_ctc_loss", dict(logits=FAKE, labels=FAKE, label_lengths=FAKE, input_lengths=None, batch=2, classes=5, length=10, max_label_len=4,
                                 blank=0, nll=FAKE, dlogits=FAKE, workspace=FAKE, workspace_bytes=1 << 40, bad_labels=None, stream=None))
SIZE = Entry("wn_ctc_workspace_bytes", dict(batch=2, classes=5, length=10, max_label_len=4))


def test_ctc_symbols_are_exported(lib):
    for entry in (LOSS, SIZE):                                       # 15 and 4 arguments
        entry.check_exported(lib)
        entry.check_declared()


def _bytes(B, T, L):
    sp = (2 * L + 1 + 63) // 64 * 64
    return B * T * 8 + 2 * B * T * sp * 8 + B * 8 + 256


def test_workspace_bytes(lib):
    for B, C, T, L in [(1, 2, 1, 1), (3, 5, 77, 31), (3, 5, 77, 32), (8, 5, 1000, 100), (32, 5, 4098, 420), (1, 64, 2304, 2047),
                       (2, MAX_CLASSES, 100, 31), (2, 5, 100, MAX_LABELS), (MAX_BATCH, 5, 100, 10), (MAX_BATCH, 5, 32768, 1)]:
        assert lib.wn_ctc_workspace_bytes(B, C, T, L) == _bytes(B, T, L), (B, C, T, L)
    assert _bytes(1, 2304, 2047) == 151_013_640                          # the 151 MB of the 2047-label test
    for B, C, T, L in [(0, 5, 100, 10), (8, 1, 100, 10), (8, 0, 100, 10), (8, 5, 0, 10), (8, 5, 100, 0), (-1, 5, 100, 10), (8, -5, 100, 10),
                       (8, 5, -100, 10), (8, 5, 100, -3), (8, MAX_CLASSES + 1, 100, 10), (8, 5, 100, MAX_LABELS + 1),
                       (MAX_BATCH + 1, 5, 100, 10), (MAX_BATCH, 5, 32769, 10), (2, 5, 2 ** 30, 10)]:
        assert lib.wn_ctc_workspace_bytes(B, C, T, L) == 0, (B, C, T, L)


def test_loss_rejects_on_the_host(lib):
    LOSS.rejects(lib, "logits",
                 shape=(dict(batch=0), dict(batch=-2), dict(classes=1), dict(classes=0), dict(length=0), dict(length=-1), dict(max_label_len=0),
                        dict(max_label_len=-1), dict(blank=5), dict(blank=-1), dict(classes=64, blank=64)),
                 unsupported=(dict(classes=MAX_CLASSES + 1), dict(max_label_len=MAX_LABELS + 1), dict(batch=MAX_BATCH + 1),
                              dict(batch=MAX_BATCH, length=32769), dict(batch=2, length=2 ** 30)),
                 required=("logits", "labels", "label_lengths", "nll", "workspace"))
    need = SIZE(lib)
    assert need == _bytes(2, 10, 4)
    assert LOSS(lib, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert LOSS(lib, workspace_bytes=0) == WN_ERR_WORKSPACE
    for off in (1, 2, 4, 7):
        assert LOSS(lib, workspace=ctypes.c_void_p((1 << 20) + off)) == WN_ERR_WORKSPACE, off      # not 8-byte aligned


def test_the_order_of_the_checks(lib):
    """shape, then unsupported, then NULL, then workspace"""
    assert LOSS(lib, batch=0, classes=65, logits=None, workspace_bytes=0) == WN_ERR_BAD_SHAPE
    assert LOSS(lib, blank=7, max_label_len=2048, logits=None, workspace_bytes=0) == WN_ERR_BAD_SHAPE
    assert LOSS(lib, classes=65, logits=None, workspace_bytes=0) == WN_ERR_UNSUPPORTED
    assert LOSS(lib, logits=None, workspace_bytes=0) == WN_ERR_NULL
    assert LOSS(lib, workspace=None, workspace_bytes=0) == WN_ERR_NULL
    assert LOSS(lib, workspace=ctypes.c_void_p((1 << 20) + 4), workspace_bytes=0) == WN_ERR_WORKSPACE


def test_the_limits_themselves_are_accepted(lib):
    """at C = 64, L = 2047, B = 65535 every check up to the workspace's passes: one byte short is the first complaint"""
    for kw in (dict(classes=MAX_CLASSES, blank=63), dict(max_label_len=MAX_LABELS), dict(batch=MAX_BATCH),
               dict(batch=MAX_BATCH, length=32768, max_label_len=1), dict(batch=1, classes=MAX_CLASSES, length=2304, max_label_len=MAX_LABELS)):
        shape = dict(SIZE.defaults, **{k: v for k, v in kw.items() if k in SIZE.defaults})
        need = SIZE(lib, **shape)
        assert need == _bytes(shape["batch"], shape["length"], shape["max_label_len"]) > 0, kw
        assert LOSS(lib, workspace_bytes=need - 1, **kw) == WN_ERR_WORKSPACE, kw


def test_the_documented_limits_match():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    line = next(l for l in text.splitlines() if "limits (checked, WN_ERR_UNSUPPORTED otherwise)" in l)
    m = re.search(r"C <= (\d+) classes, Lmax <= (\d+) labels per utterance, B <= (\d+), B\*T < 2\^(\d+)", line)
    assert m, line
    assert tuple(int(v) for v in m.groups()) == (MAX_CLASSES, MAX_LABELS, MAX_BATCH, 31)
