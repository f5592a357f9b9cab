"""CPU (hipcc cross-compiles without a GPU): no kernel of csrc/wn_readmap.hip uses scratch (register spills), checked on the
metadata of the generated gfx950 assembly."""
import re

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_readmap_kernels_use_no_scratch():
    text = open(listing("wn_readmap.hip")).read()
    names = re.findall(r"\.name:\s+(_Z\S*(?:minimizer|read_seeds|chain)_kernel\S*)", text)
    assert len(names) == 3, names                                    # sketch, seeds, chain
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 3 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
    assert "v_readlane_b32" in text and "row_bcast:31" in text       # the chain's wave maximum is DPP, its broadcast a readlane
