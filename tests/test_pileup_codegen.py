"""CPU (hipcc cross-compiles without a GPU): csrc/wn_pileup.hip compiles for gfx950 and no kernel of it uses scratch (register
spills, indexed local arrays), checked on the metadata of the generated assembly."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_pileup_kernels_use_no_scratch():
    out = os.path.join(tempfile.mkdtemp(prefix="wn_asm_"), "wn_pileup.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "wavenet_speech_amd", "csrc", "wn_pileup.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    names = re.findall(r"\.name:\s+(_Z\S*(?:pileup|consensus_call|consensus_scan|consensus_emit)_kernel\S*)", text)
    assert len(names) == 4, names                                    # pileup, call, scan of the tile totals, emit
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 4 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
    assert "global_atomic_add" in text                               # the tables are added into with integer atomics
