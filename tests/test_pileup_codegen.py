"""CPU (hipcc cross-compiles without a GPU): csrc/wn_pileup.hip compiles for gfx950 and no kernel of it uses scratch (register
spills, indexed local arrays), checked on the metadata of the generated assembly."""
import re

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_pileup_kernels_use_no_scratch():
    text = open(listing("wn_pileup.hip")).read()
    names = re.findall(r"\.name:\s+(_Z\S*(?:pileup|consensus_call|consensus_scan|consensus_emit)_kernel\S*)", text)
    assert len(names) == 4, names                                    # pileup, call, scan of the tile totals, emit
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 4 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
    assert "global_atomic_add" in text                               # the tables are added into with integer atomics
