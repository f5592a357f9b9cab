"""CPU (hipcc cross-compiles without a GPU): every csrc file that takes its wave and workgroup steps from csrc/wn_wave_dev.h compiles
for gfx950, still holds the kernels it held before the steps moved there, and no kernel of it uses scratch (register spills, indexed
local arrays), checked on the metadata of the generated assembly.  wn_pileup.hip takes the walk over an op row from
csrc/wn_opscan.h through lambdas: the same two properties hold it (tests/test_genotype_codegen.py holds wn_genotype.hip, the other
file on that walk)."""
import re

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")

# kernels per file, counted in the assembly of the commit before the shared header
KERNELS = {"wn_reads.hip": 2, "wn_readmap.hip": 3, "wn_select.hip": 8, "wn_pileup.hip": 4, "wn_profile.hip": 1, "wn_eventdetect.hip": 5,
           "wn_demux.hip": 5, "wn_events.hip": 3, "wn_align.hip": 2, "wn_pairalign.hip": 2}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_kernels_are_all_there_and_use_no_scratch(name):
    text = open(listing(name)).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    assert len(kernels) == KERNELS[name], kernels
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == KERNELS[name] and all(int(x) == 0 for x in sizes), "scratch in use: %s" % sizes
