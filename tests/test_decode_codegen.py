"""CPU (hipcc cross-compiles without a GPU): no kernel of csrc/wn_decode.hip uses scratch (register spills), checked on the
generated gfx950 assembly."""
import re

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_decode_kernels_use_no_scratch():
    text = open(listing("wn_decode.hip")).read()
    names = re.findall(r"\.name:\s+(_Z\S*ctc_\w*kernel\S*)", text)
    assert len(names) == 3, names                                    # greedy, beam, beam walk
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert sizes and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
    assert "scratch_store" not in text and "scratch_load" not in text
