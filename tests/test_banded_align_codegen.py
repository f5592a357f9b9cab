"""CPU (hipcc cross-compiles without a GPU): both forms of band_align_kernel (csrc/wn_bandalign.hip) compile for gfx950 without
scratch and without register spills -- the 24 H / E / F values of a thread stay in registers -- and the neighbour exchange of
the one-wave form is DPP both ways.  By the recipe of tools/listing.py."""
import re

import pytest

from tools.listing import NO_HIPCC, kernels, listing, resources

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_both_forms_use_no_scratch_and_spill_nothing():
    found = kernels(open(listing("wn_bandalign.hip")).read())
    assert len(found) == 2 and all("band_align_kernel" in name for name, _ in found), found      # one wave, and 256 threads
    assert all(size == 0 for _, size in found), "scratch in use: %s" % found
    rows = resources("wn_bandalign.hip")
    assert len(rows) == 2, rows
    for row in rows:
        assert row["ScratchSize [bytes/lane]"] == "0" and row["VGPRs Spill"] == "0" and row["SGPRs Spill"] == "0", row
        assert int(row["VGPRs"]) <= 128, row                         # and no form is near the limit of its launch bounds


def test_the_one_wave_form_exchanges_by_dpp_and_has_no_barrier_in_its_step():
    text = open(listing("wn_bandalign.hip")).read()
    one, multi = [re.search(r"^(%s):[^\n]*\n(.*?)\.Lfunc_end" % re.escape(name), text, re.S | re.M).group(2)
                  for name in sorted(n for n, _ in kernels(text))]   # ILb0E sorts before ILb1E
    assert "wave_shr:1" in one and "wave_shl:1" in one
    assert "wave_shr:1" in multi and "wave_shl:1" in multi
    # a barrier of a single wave is no s_barrier instruction at all; the 256-thread form has its one per step (and the trace's)
    assert "s_barrier" not in one
    assert "s_barrier" in multi
