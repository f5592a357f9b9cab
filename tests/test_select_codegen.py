"""CPU (hipcc cross-compiles without a GPU): csrc/wn_select.hip compiles for gfx950 and none of its kernels uses scratch,
checked on the generated assembly."""
import re

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_select_kernels_use_no_scratch():
    text = open(listing("wn_select.hip")).read()
    names = re.findall(r"\.name:\s+(_Z\S*select_(?:pass|final)_kernel\S*)", text)
    assert len(names) == 8, names                                    # pass and final kernel, int16 / fp32, with and without center
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 8 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
