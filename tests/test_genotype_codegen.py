"""CPU (hipcc cross-compiles without a GPU): csrc/wn_genotype.hip compiles for gfx950, holds two kernels and neither uses scratch
(register spills, indexed local arrays), checked on the metadata of the generated assembly."""
import re

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_genotype_kernels_use_no_scratch():
    text = open(listing("wn_genotype.hip")).read()
    names = re.findall(r"\.name:\s+(_Z\S*(?:pileup_evidence|genotype_call)_kernel\S*)", text)
    assert len(names) == 2, names                                    # the evidence walk and the call
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 2 and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
    assert "global_atomic_add_x2" in text                            # the evidence is added into with 64-bit integer atomics
    kernarg = [int(x) for x in re.findall(r"\.kernarg_segment_size:\s*(\d+)", text)]
    assert max(kernarg) >= 3 * 94 * 4                                # the weight table travels in the kernel arguments
