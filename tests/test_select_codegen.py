"""CPU (hipcc cross-compiles without a GPU): csrc/wn_select.hip compiles for gfx950 and none of its kernels uses scratch,
checked on the generated assembly."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_select_kernels_use_no_scratch():
    out = os.path.join(tempfile.mkdtemp(prefix="wn_asm_"), "wn_select.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "wavenet_speech_amd", "csrc", "wn_select.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    names = re.findall(r"\.name:\s+(_Z\S*select_(?:pass|final)_kernel\S*)", text)
    assert len(names) == 8, names                                    # pass and final kernel, int16 / fp32, with and without center
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 8 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
