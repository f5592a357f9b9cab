"""CPU (hipcc cross-compiles without a GPU): csrc/wn_align.hip compiles for gfx950 and none of its kernels uses scratch
(register spills: the per-thread state arrays must stay in registers), checked on the generated assembly."""
import re

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_align_kernels_use_no_scratch():
    text = open(listing("wn_align.hip")).read()
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
