"""CPU (hipcc cross-compiles without a GPU): csrc/wn_leftalign.hip compiles for gfx950, holds its one kernel, and that kernel uses no
scratch (register spills, indexed local arrays) and no floating point, checked on the generated assembly."""
import os
import re

import pytest

from tools.listing import NO_HIPCC, ROOT, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")


def test_left_align_kernel_uses_no_scratch_and_no_floating_point():
    text = open(listing("wn_leftalign.hip")).read()
    names = re.findall(r"\.name:\s+(_Z\S*_kernel\S*)", text)
    assert len(names) == 1 and "left_align_kernel" in names[0], names
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 1 and int(sizes[0]) == 0, "scratch in use: %s" % sizes
    assert not re.search(r"^\s+v_\w+_f(16|32|64)\b", text, flags=re.M)     # labels and ops are only compared
    assert "s_barrier" in text                                       # the passes meet inside the one launch


def test_the_makefile_builds_the_file():
    text = open(os.path.join(ROOT, "wavenet_speech_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bwn_leftalign\.hip\b", text, flags=re.M)
