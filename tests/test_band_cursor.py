"""CPU (hipcc compiles for the host and cross-compiles without a GPU): the banded-path core that signal_align and event_align
share (csrc/wn_band_dev.h).  Its incremental band cursor is held to the closed form band_lo by a host program, and the two kernels
built on it keep their per-slot state in registers: no scratch, checked on the metadata of the generated gfx950 assembly."""
import os
import re
import subprocess
import tempfile

import pytest

from tools.listing import HIPCC, NO_HIPCC, ROOT, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_cursor_matches_closed_form():
    """advance() == band_lo(i) - band_lo(i - 1) and lo_slot == lo % W at every step of W in {64, 128}, n in 1..200,
    N in 1..3 (n - 1) + 1: N <= W, N = n, N = 3 (n - 1) + 1 and every delta 0..3 (tests/band_cursor_check.cpp)"""
    exe = os.path.join(tempfile.mkdtemp(prefix="wn_band_"), "band_cursor_check")
    r = subprocess.run([HIPCC, "-O2", "-std=c++20", "-x", "hip", "--offload-host-only", os.path.join(ROOT, "tests", "band_cursor_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.match(r"steps (\d+) deltas 0x([0-9a-f]+)", r.stdout)
    # 2 sum_{m = 0..199} m (3 m + 1) steps: the whole grid was walked, and every delta was met
    assert m and int(m.group(1)) == 15_920_000 and int(m.group(2), 16) == 0xf, r.stdout


def test_band_kernels_use_no_scratch():
    found = {}
    for src in ("wn_sigalign.hip", "wn_eventalign.hip"):
        text = open(listing(src)).read()
        names = re.findall(r"\.name:\s+(_Z\S*(?:signal|event)_align_kernel\S*)", text)
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
        assert len(names) == len(sizes), (names, sizes)
        found.update(zip(names, (int(x) for x in sizes)))
    # Itanium names: signal_align_kernel<float> is ...kernelIfE..., <short> ...kernelIsE..., event_align_kernel is no template
    kernels = sorted(re.search(r"(?:signal|event)_align_kernel(?:I\w+?E)?", n).group(0) for n in found)
    assert kernels == ["event_align_kernel", "signal_align_kernelIfE", "signal_align_kernelIsE"], sorted(found)
    assert all(v == 0 for v in found.values()), "scratch in use: %s" % found
