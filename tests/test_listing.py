"""CPU (hipcc cross-compiles without a GPU): tools/listing.py compiles a file once per process, reads the kernels out of the
listing, and gets its command line -- the per-file flags included -- from csrc/Makefile."""
import os
import re
import subprocess

import pytest

from tools import listing as L

pytestmark = pytest.mark.skipif(L.NO_HIPCC, reason="hipcc not installed")


def test_a_file_is_compiled_once_and_its_kernels_are_read():
    L._DONE.pop(("listing", L.CSRC, "wn_pack.hip"), None)             # another test of the session may have come first
    before = L.compiles
    first = L.listing("wn_pack.hip")
    assert L.listing("wn_pack.hip") == first and os.path.exists(first)
    assert L.compiles - before == 1
    found = L.kernels(open(first).read())
    assert len(found) >= 1 and all(isinstance(size, int) for _, size in found), found


def test_the_per_file_flags_come_from_the_makefile():
    value = re.search(r"^FLAGS_wn_col2\s*=\s*(\S.*)$", open(os.path.join(L.CSRC, "Makefile")).read(), re.M).group(1).strip()

    def command(src):
        return subprocess.run(["make", "-n", "-C", L.CSRC, "listing", "SRC=" + src, "OUT=/dev/null"], capture_output=True, text=True,
                              check=True).stdout

    assert value and set(value.split()) <= set(command("wn_col2.hip").split())
    assert not set(value.split()) & set(command("wn_pack.hip").split()) and "wn_pack.hip" in command("wn_pack.hip")
