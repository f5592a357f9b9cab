"""CPU (hipcc cross-compiles without a GPU): csrc/wn_realign.hip compiles for gfx950, holds its two kernels, neither uses scratch
(register spills, indexed local arrays) or spills a register, and their LDS is the scan slots and the reduction rows only -- a few
hundred bytes whatever the window or the rows hold -- checked on the metadata of the generated assembly."""
import re

import pytest

from tools.listing import NO_HIPCC, kernels, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")
KERNELS = ("haplotype_windows", "lift_ops")
# haplotype_windows: s_scan[2][2][4] and s_sum[4][5] ints; lift_ops: the walk's s_slot[2][2][4], lo / hi / bad twice, s_scan[2][4], s_sum[4][5]
LDS_BOUND = {"haplotype_windows": (16 + 20) * 4, "lift_ops": (16 + 6 + 8 + 20) * 4}
PADDING = 32


def _meta(text):
    """{kernel: its metadata block} from the amdhsa.kernels notes"""
    blocks = re.split(r"\n  - \.agpr_count:", text[text.index("amdhsa.kernels:"):])[1:]
    out = {}
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        for k in KERNELS:
            if "%d%s_kernel" % (len(k) + 7, k) in name:
                out[k] = b
    return out


def test_realign_kernels_use_no_scratch_no_spills_and_little_lds():
    text = open(listing("wn_realign.hip")).read()
    assert len(kernels(text)) == len(KERNELS) and all(scratch == 0 for _, scratch in kernels(text)), kernels(text)
    meta = _meta(text)
    assert sorted(meta) == sorted(KERNELS), sorted(meta)
    for k, b in meta.items():
        field = lambda name: int(re.search(r"\.%s:\s*(\d+)" % name, b).group(1))      # noqa: E731
        assert field("private_segment_fixed_size") == 0, "scratch in %s" % k
        assert field("sgpr_spill_count") == 0 and field("vgpr_spill_count") == 0, "spills in %s" % k
        assert 0 < field("group_segment_fixed_size") <= LDS_BOUND[k] + PADDING, (k, field("group_segment_fixed_size"))
        assert field("max_flat_workgroup_size") == 256
