"""CPU (hipcc cross-compiles without a GPU): csrc/wn_cigar.hip compiles for gfx950 by the recipe of tools/listing.py, holds its two
kernels, and neither uses scratch, spills a register or touches floating point."""
import os
import re

import pytest

from tools.listing import NO_HIPCC, ROOT, kernels, listing, resources

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_both_kernels_use_no_scratch_and_no_floating_point():
    text = open(listing("wn_cigar.hip")).read()
    found = kernels(text)
    assert len(found) == 2 and "cigar_encode_kernel" in found[0][0] and "cigar_decode_kernel" in found[1][0], found
    assert [size for _, size in found] == [0, 0], "scratch in use: %s" % found
    assert not re.search(r"^\s+v_\w+_f(16|32|64)\b", text, flags=re.M)     # runs, ops and labels are integers
    assert "s_barrier" in text                                       # the waves of a read meet inside the one launch


def test_no_kernel_spills():
    rows = resources("wn_cigar.hip")
    assert len(rows) == 2 and all("cigar_" in r["Function Name"] for r in rows), rows
    for r in rows:
        assert (r["ScratchSize [bytes/lane]"], r["SGPRs Spill"], r["VGPRs Spill"]) == ("0", "0", "0"), r
        assert int(r["Occupancy [waves/SIMD]"]) >= 8 and int(r["LDS Size [bytes/block]"]) <= 1024, r


def test_the_makefile_builds_the_file():
    text = open(os.path.join(ROOT, "wavenet_speech_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwn_cigar\.hip\b", text, flags=re.M)
