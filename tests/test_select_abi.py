"""CPU: the C ABI of read selection (csrc/wn_select.hip): exported symbols, the ctypes table against the header, the workspace
size, and the shape / limit / pointer / workspace checks, which run on the host before any HIP call -- none of the calls below
touches a device."""
import ctypes
import os
import re

from tests.abi_util import FAKE, ROOT, WN_ERR_BAD_SHAPE, WN_ERR_NULL, WN_ERR_UNSUPPORTED, WN_ERR_WORKSPACE, Entry
from tests.abi_util import lib  # noqa: F401

ODD = ctypes.c_void_p((1 << 20) + 8)     # 8-byte but not 16-byte aligned
EDGE = 2 ** 31 - 1024                    # the first ld that is refused
BIG = 1 << 40                            # a workspace size that is always enough
SELECT = Entry("wn_read_select", dict(signal=FAKE, signal_is_int16=0, batch=2, ld=100, signal_lengths=FAKE, ranks=FAKE, K=2, center=None, out=FAKE,
                                      workspace=FAKE, workspace_bytes=BIG, bad=None, stream=None))
SIZE = Entry("wn_read_select_workspace_bytes", dict(batch=2, K=2, signal_is_int16=0, has_center=0))
REQUIRED = ("signal", "signal_lengths", "ranks", "out", "workspace")       # center and bad are optional (NULL in every call here)


def test_select_symbols_are_exported(lib):
    SELECT.check_exported(lib)
    SIZE.check_exported(lib)


def test_signature_table_matches_the_header():
    SELECT.check_declared()                                          # 13 arguments
    SIZE.check_declared()                                            # 4


def test_tile_matches_the_kernel():
    from wavenet_speech_amd import normalise
    src = open(os.path.join(ROOT, "wavenet_speech_amd", "csrc", "wn_select.hip")).read()
    assert int(re.search(r"constexpr int kSelTile = (\d+);", src).group(1)) == normalise.TILE
    assert int(re.search(r"constexpr int kSelMaxK = (\d+);", src).group(1)) == normalise.MAX_RANKS


def test_workspace_bytes(lib):
    ws = lib.wn_read_select_workspace_bytes
    # per read: one histogram of 256 uint32 for the first pass, K for every later one; int16 without center has 2 passes, else 4
    assert ws(1, 1, 1, 0) == 2 * 1024 and ws(1, 1, 0, 0) == 4 * 1024
    assert ws(3, 2, 1, 0) == 3 * (1 + 2) * 1024
    assert ws(3, 2, 1, 1) == ws(3, 2, 0, 0) == ws(3, 2, 0, 1) == 3 * (1 + 3 * 2) * 1024
    assert ws(65535, 8, 0, 1) == 65535 * 25 * 1024                   # above 2^30: a size_t
    for batch, K in ((1, 1), (65535, 1), (1, 8), (48, 2)):
        for is_int16 in (0, 1):
            for has_center in (0, 1):
                assert ws(batch, K, is_int16, has_center) > 0
    for batch, K in ((0, 1), (-1, 1), (65536, 1), (1, 0), (1, -2), (1, 9)):
        assert ws(batch, K, 1, 0) == 0 and ws(batch, K, 0, 1) == 0


def test_read_select_rejects_on_the_host(lib):
    SELECT.rejects(lib, "out", shape=(dict(batch=0), dict(batch=-1), dict(ld=0), dict(ld=-7), dict(K=0), dict(K=-3)),
                   unsupported=(dict(K=9), dict(batch=65536), dict(ld=EDGE),
                                # a launch stays below 2^32 threads: 256 * ceil(ld / 8192) * batch
                                dict(ld=8192 * 512, batch=32768),                              # 2^32
                                dict(ld=8192 * 256 + 1, batch=65535)),
                   accepted=(dict(K=8), dict(K=1), dict(batch=65535), dict(batch=1, ld=1), dict(batch=1, ld=EDGE - 1),
                             dict(ld=8192 * 256, batch=65535),                                 # 2^32 - 2^16
                             dict(ld=8192 * 512, batch=32767)),
                   required=REQUIRED)
    for name in REQUIRED:
        assert SELECT(lib, signal_is_int16=1, **{name: None}) == WN_ERR_NULL, name
    # the workspace: 16-byte aligned and at least wn_read_select_workspace_bytes
    assert SELECT(lib, workspace=ODD) == WN_ERR_WORKSPACE
    assert SELECT(lib, workspace=ctypes.c_void_p((1 << 20) + 4)) == WN_ERR_WORKSPACE
    for is_int16 in (0, 1):
        for center in (None, FAKE):
            need = SIZE(lib, signal_is_int16=is_int16, has_center=int(center is not None))
            assert SELECT(lib, signal_is_int16=is_int16, center=center, workspace_bytes=need - 1) == WN_ERR_WORKSPACE
    assert SELECT(lib, workspace_bytes=0) == WN_ERR_WORKSPACE
    # a signal that is not aligned to its element could not be read 16 bytes at a time from any boundary
    assert SELECT(lib, signal_is_int16=1, signal=ctypes.c_void_p((1 << 20) + 1)) == WN_ERR_WORKSPACE
    assert SELECT(lib, signal_is_int16=0, signal=ctypes.c_void_p((1 << 20) + 2)) == WN_ERR_WORKSPACE
    # the order of the checks: shape, then unsupported, then NULL, then the workspace
    assert SELECT(lib, K=0, batch=65536, ranks=None) == WN_ERR_BAD_SHAPE
    assert SELECT(lib, batch=0, ld=EDGE, ranks=None) == WN_ERR_BAD_SHAPE
    assert SELECT(lib, K=9, ranks=None, workspace=ODD) == WN_ERR_UNSUPPORTED
    assert SELECT(lib, ld=EDGE, signal=None) == WN_ERR_UNSUPPORTED
    assert SELECT(lib, ranks=None, workspace=ODD) == WN_ERR_NULL
    assert SELECT(lib, ranks=None, workspace_bytes=0) == WN_ERR_NULL
