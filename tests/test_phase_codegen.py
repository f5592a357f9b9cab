"""CPU (hipcc cross-compiles without a GPU): csrc/wn_phase.hip compiles for gfx950, holds its six kernels, none uses scratch
(register spills, indexed local arrays), the links are added with 64-bit integer atomics, and the link kernel's LDS stays within
the 16 KB of an observation per window position plus the walk's slots -- checked on the metadata of the generated assembly."""
import re

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")
KERNELS = ("phase_links", "haplotag", "phase_parent", "phase_jump", "phase_root", "phase_size")
WALK_SLOTS = 2 * 2 * 4 * 4 + 3 * 4            # s_slot[2][2][4] and lo, hi, bad


def _kernels(text):
    """{kernel: its metadata block} from the amdhsa.kernels notes"""
    blocks = re.split(r"\n  - \.agpr_count:", text[text.index("amdhsa.kernels:"):])[1:]
    out = {}
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        for k in KERNELS:
            if "%d%s_kernel" % (len(k) + 7, k) in name:
                out[k] = b
    return out


def test_phase_kernels_use_no_scratch_and_little_lds():
    text = open(listing("wn_phase.hip")).read()
    meta = _kernels(text)
    assert sorted(meta) == sorted(KERNELS), sorted(meta)
    for k, b in meta.items():
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", b).group(1)) == 0, "scratch in %s" % k
    lds = {k: int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", b).group(1)) for k, b in meta.items()}
    assert 0 < lds["phase_links"] <= 16384 + WALK_SLOTS + 64, lds    # 64: the observation counts of the waves, and padding
    assert lds["phase_parent"] == lds["phase_jump"] == lds["phase_root"] == lds["phase_size"] == 0


def test_the_links_are_added_with_64_bit_atomics():
    text = open(listing("wn_phase.hip")).read()
    start = text.index("phase_links_kernel")
    body = text[start:text.index(".end_amdhsa_kernel", start)]
    assert "global_atomic_add_x2" in body                            # links: one 64-bit add with its carry
    assert "global_atomic_add " in body or "global_atomic_add\t" in body     # observed: 32-bit counts
