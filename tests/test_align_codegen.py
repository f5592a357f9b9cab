"""CPU (hipcc cross-compiles without a GPU): csrc/wn_align.hip compiles for gfx950 and none of its kernels uses scratch
(register spills: the per-thread state arrays must stay in registers), checked on the generated assembly."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_align_kernels_use_no_scratch():
    out = os.path.join(tempfile.mkdtemp(prefix="wn_asm_"), "wn_align.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "wavenet_speech_amd", "csrc", "wn_align.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    names = re.findall(r"\.name:\s+(_Z\S*ctc_align_kernel\S*)", text)
    assert len(names) == 2, names                                    # one wave (<= 255 labels) and up to eight waves
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 2 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
    assert "scratch_store" not in text and "scratch_load" not in text
    # the neighbour's state crosses lanes by a DPP wavefront shift, not through LDS
    assert "wave_shr:1" in text
    # stores to memory are vector stores: no scalar-memory write of any kind
    scalar_mem = re.findall(r"^\s+(s_\w+)", text, flags=re.M)
    assert not [m for m in scalar_mem if "store" in m or "atomic" in m or "dcache" in m]
