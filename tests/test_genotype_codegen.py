"""CPU (hipcc cross-compiles without a GPU): csrc/wn_genotype.hip compiles for gfx950, holds two kernels and neither uses scratch
(register spills, indexed local arrays), checked on the metadata of the generated assembly."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_genotype_kernels_use_no_scratch():
    out = os.path.join(tempfile.mkdtemp(prefix="wn_asm_"), "wn_genotype.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "wavenet_speech_amd", "csrc", "wn_genotype.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    names = re.findall(r"\.name:\s+(_Z\S*(?:pileup_evidence|genotype_call)_kernel\S*)", text)
    assert len(names) == 2, names                                    # the evidence walk and the call
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 2 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
    assert "global_atomic_add_x2" in text                            # the evidence is added into with 64-bit integer atomics
    kernarg = [int(x) for x in re.findall(r"\.kernarg_segment_size:\s*(\d+)", text)]
    assert max(kernarg) >= 3 * 94 * 4                                # the weight table travels in the kernel arguments
