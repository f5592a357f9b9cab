"""CPU: the weight-gradient groups of the half-precision backward (functional_half.wgrad_groups) on stacks whose blocks differ in
kernel width or width.  Every group it forms must be one the library can plan (wn_hblocks_wgrad_workspace_bytes > 0): a group
of eight k=3 blocks needs 24 pairs of the 19 a launch holds, and planning from the bottom block alone formed one."""
import ctypes

import pytest

from wavenet_speech_amd import _lib
from wavenet_speech_amd.functional import BlockSpec
from wavenet_speech_amd.functional_half import HalfLayout, _shape, wgrad_groups

DILATIONS = [1, 2, 4, 8, 16, 32, 64] * 3


def _notebook(c):
    """the reference's training model (RawCTCNet, causal, input block k=2 d=1): 21 blocks of k=2, then 21 of k=3"""
    return [(c, c, 2, 1)] + [(c, c, 2, d) for d in DILATIONS] + [(c, c, 3, d) for d in DILATIONS]


STACKS = {
    "notebook64": (_notebook(64), 64),
    "notebook128": (_notebook(128), 128),
    "notebook512": (_notebook(512), 512),
    "alternating_k64": ([(64, 64, 2 + (i % 2), 2 ** (i % 5)) for i in range(16)], 64),
    "widening_block_under_wide": ([(64, 256, 2, 1)] + [(256, 256, 2, 2 ** i) for i in range(7)], 256),
    "narrow_under_wide": ([(64, 64, 2, 1), (64, 256, 2, 2)] + [(256, 256, 2, 2 ** i) for i in range(2, 8)], 64),
    "wide_in_the_middle": ([(64, 64, 3, 1), (64, 256, 2, 2), (256, 256, 3, 4), (256, 64, 2, 8)]
                           + [(64, 64, 2 + (i % 2), 2 ** i) for i in range(8)], 64),
    "uniform_k2_64": ([(64, 64, 2, 2 ** (i % 7)) for i in range(19)], 64),
    "ci_ne_co_k3": ([(24, 40, 3, 1), (40, 40, 2, 7), (40, 72, 2, 300), (72, 72, 3, 2)], 36),
}


def _shapes(layers, ms, B=8, L=117, causal=True):
    specs = [BlockSpec(ci, co, ms, k, d, causal) for ci, co, k, d in layers]
    layout = HalfLayout(L, max(s.reach() for s in specs))
    return [_shape(s, B, layout) for s in specs]


@pytest.mark.parametrize("precision", ["bf16", "f16", "f16x3"])
@pytest.mark.parametrize("name", sorted(STACKS))
def test_every_weight_gradient_group_is_planned(name, precision):
    lib = _lib.load()
    code = _lib.PRECISIONS[precision]
    layers, ms = STACKS[name]
    shapes = _shapes(layers, ms)
    order = list(range(len(shapes) - 1, -1, -1))                 # backward reaches the top block first
    seen = []
    for cap in (None, 3, 1):
        groups = wgrad_groups(lib, [shapes[l] for l in order], code, cap)
        pos = [p for _, ps in groups for p in ps]
        assert pos == list(range(len(shapes))), groups          # every block exactly once, in the order backward reaches it
        for grouped, ps in groups:
            blocks = [shapes[order[p]] for p in ps]
            if not grouped:
                assert len(ps) == 1
                assert cap == 1 or lib.wn_hblocks_wgrad_group_max(ctypes.byref(blocks[0]), code) == 1
                assert lib.wn_hblock_wgrad_workspace_bytes(ctypes.byref(blocks[0]), code) > 0
                continue
            limit = min(lib.wn_hblocks_wgrad_group_max(ctypes.byref(s), code) for s in blocks)
            assert 1 <= len(ps) <= min(limit, cap or limit), (ps, limit)
            arr = (_lib.BlockShape * len(blocks))(*blocks)
            assert lib.wn_hblocks_wgrad_workspace_bytes(arr, len(blocks), code) > 0, (name, ps)
        seen.append(groups)
    if all(co <= 128 for _ci, co, _k, _d in layers) and ms <= 128:
        assert any(len(ps) > 1 for _, ps in seen[0]), seen[0]   # small blocks are still grouped


def test_uniform_stacks_keep_their_groups():
    """equal blocks: groups of the library's limit from the top, the remainder last (the grouping of earlier releases)"""
    lib = _lib.load()
    code = _lib.PRECISIONS["bf16"]
    for k, n in ((2, 19), (3, 13), (2, 5)):
        shapes = _shapes([(64, 64, k, 2 ** (i % 6)) for i in range(n)], 64)
        limit = lib.wn_hblocks_wgrad_group_max(ctypes.byref(shapes[0]), code)
        groups = wgrad_groups(lib, shapes[::-1], code)
        want = [list(range(i, min(i + limit, n))) for i in range(0, n, limit)]
        assert [ps for _, ps in groups] == want and all(g for g, _ in groups)
    wide = _shapes([(256, 256, 2, 2 ** i) for i in range(4)], 256)
    assert wgrad_groups(lib, wide[::-1], code) == [(False, [i]) for i in range(4)]


def test_the_bottom_block_alone_does_not_plan_the_notebook_stack():
    """what the grouping of earlier releases did (one limit for the whole stack, from its bottom block): the top eight k=3
    blocks of the 64-channel notebook stack form a group the library cannot plan"""
    lib = _lib.load()
    code = _lib.PRECISIONS["bf16"]
    shapes = _shapes(_notebook(64), 64)
    limit = lib.wn_hblocks_wgrad_group_max(ctypes.byref(shapes[0]), code)
    top = (_lib.BlockShape * limit)(*shapes[::-1][:limit])
    assert limit == 8 and lib.wn_hblocks_wgrad_workspace_bytes(top, limit, code) == 0
    # and a 64-channel block under 256-channel ones: the bottom block's limit groups the wide blocks' ordinary pairs
    layers, ms = STACKS["narrow_under_wide"]
    shapes = _shapes(layers, ms)
    limit = lib.wn_hblocks_wgrad_group_max(ctypes.byref(shapes[0]), code)
    top = (_lib.BlockShape * limit)(*shapes[::-1][:limit])
    assert limit == 8 and lib.wn_hblocks_wgrad_workspace_bytes(top, limit, code) == 0
