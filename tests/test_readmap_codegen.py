"""CPU (hipcc cross-compiles without a GPU): no kernel of csrc/wn_readmap.hip uses scratch (register spills), checked on the
metadata of the generated gfx950 assembly."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_readmap_kernels_use_no_scratch():
    out = os.path.join(tempfile.mkdtemp(prefix="wn_asm_"), "wn_readmap.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "wavenet_speech_amd", "csrc", "wn_readmap.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    names = re.findall(r"\.name:\s+(_Z\S*(?:minimizer|read_seeds|chain)_kernel\S*)", text)
    assert len(names) == 3, names                                    # sketch, seeds, chain
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 3 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
    assert "v_readlane_b32" in text and "row_bcast:31" in text       # the chain's wave maximum is DPP, its broadcast a readlane
