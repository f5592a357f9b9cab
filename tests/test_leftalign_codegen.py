"""CPU (hipcc cross-compiles without a GPU): csrc/wn_leftalign.hip compiles for gfx950, holds its one kernel, and that kernel uses no
scratch (register spills, indexed local arrays) and no floating point, checked on the generated assembly."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_left_align_kernel_uses_no_scratch_and_no_floating_point():
    out = os.path.join(tempfile.mkdtemp(prefix="wn_asm_"), "wn_leftalign.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "wavenet_speech_amd", "csrc", "wn_leftalign.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    names = re.findall(r"\.name:\s+(_Z\S*_kernel\S*)", text)
    assert len(names) == 1 and "left_align_kernel" in names[0], names
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 1 and int(sizes[0]) == 0, "scratch in use: %s" % sizes
    assert not re.search(r"^\s+v_\w+_f(16|32|64)\b", text, flags=re.M)     # labels and ops are only compared
    assert "s_barrier" in text                                       # the passes meet inside the one launch


def test_the_makefile_builds_the_file():
    text = open(os.path.join(ROOT, "wavenet_speech_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwn_leftalign\.hip\b", text, flags=re.M)
