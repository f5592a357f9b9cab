"""GPU: one pack launch per fp32 stack (functional.StackPackTable over wn_stack_pack_*) writes, at the offsets the table reports,
byte for byte the images of the per-object entry points (wn_block_pack, wn_skipsum_pack, wn_conv_pack)."""
import ctypes

import pytest
import torch

from wavenet_speech_amd import _lib
from wavenet_speech_amd import functional as HF
from wavenet_speech_amd.functional import BlockSpec, StackPackTable, _p, _params_struct, _prep_params, _shape, _stream
from wavenet_speech_amd.series import SeriesLayout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, MS, B = 40, 24, 2
STACKS = {
    "mixed_k2_k3": [(C, C, 2, 1), (C, C, 3, 2), (C, C, 2, 4)],
    "one_k3": [(C, C, 3, 2)],
}


def _params(blocks, gen):
    """ten nn.Parameters per block (C-ABI order); the skip projections and their biases as slices of two plain tensors, as the
    folded bottleneck x skip products arrive in a model"""
    n = len(blocks)
    wf = torch.randn(n, MS, C, generator=gen).to(DEV)
    bf = torch.randn(n, MS, generator=gen).to(DEV)
    flat = []
    for l, (ci, co, k, _d) in enumerate(blocks):
        shapes = [(co, ci, k), (co,), (co, ci, k), (co,), (co, co, 1), (co,), None, None, (co, ci), (co,)]
        for i, shp in enumerate(shapes):
            if i == 6:
                flat.append(wf[l])
            elif i == 7:
                flat.append(bf[l])
            else:
                flat.append(torch.nn.Parameter(torch.randn(*shp, generator=gen).to(DEV)))
    return flat, wf, bf


def _reference_images(lib, specs, layout, prepped, bias_total, convs):
    """the per-object packs into zeroed buffers (the padding between an image's weights and biases is never written)"""
    blocks, skipsum, cimgs = [], None, []
    for spec, prm in zip(specs, prepped):
        shape = _shape(spec, B, layout)
        buf = torch.zeros(lib.wn_block_packed_bytes(ctypes.byref(shape)), dtype=torch.uint8, device=DEV)
        ps = _params_struct(prm)
        _lib.check(lib.wn_block_pack(ctypes.byref(shape), ctypes.byref(ps), _p(buf), _stream()), "wn_block_pack")
        blocks.append(buf)
    if bias_total is not None:
        idx = range(len(specs))
        shape = HF._skipsum_shape(specs, idx, B, layout)
        skipsum = torch.zeros(lib.wn_skipsum_packed_bytes(ctypes.byref(shape)), dtype=torch.uint8, device=DEV)
        wptrs = (ctypes.c_void_p * len(specs))(*[p[6].data_ptr() for p in prepped])
        _lib.check(lib.wn_skipsum_pack(ctypes.byref(shape), wptrs, _p(bias_total), _p(skipsum), _stream()), "wn_skipsum_pack")
    for sh, w, b in convs:
        buf = torch.zeros(lib.wn_conv_packed_bytes(ctypes.byref(sh)), dtype=torch.uint8, device=DEV)
        _lib.check(lib.wn_conv_pack(ctypes.byref(sh), _p(w), _p(b), _p(buf), _stream()), "wn_conv_pack")
        cimgs.append(buf)
    return blocks, skipsum, cimgs


def _check_images(table, packed, blocks, skipsum, cimgs):
    ends = []
    for off, img in zip(table.block_offsets, blocks):
        assert torch.equal(packed[off:off + img.numel()], img)
        ends.append(off + img.numel())
    if skipsum is not None:
        off = table.skipsum_offsets[0]
        assert torch.equal(packed[off:off + skipsum.numel()], skipsum)
        ends.append(off + skipsum.numel())
    for off, img in zip(table.conv_offsets, cimgs):
        assert torch.equal(packed[off:off + img.numel()], img)
        ends.append(off + img.numel())
    assert max(ends) == table.total == packed.numel()


@pytest.mark.parametrize("L", [130, 5])
@pytest.mark.parametrize("stack", sorted(STACKS))
@pytest.mark.parametrize("training", [True, False])
def test_stack_image_is_the_per_object_images(stack, L, training):
    lib = _lib.load()
    gen = torch.Generator().manual_seed(L + len(stack))
    blocks = STACKS[stack]
    specs = [BlockSpec(ci, co, MS, k, d, True) for ci, co, k, d in blocks]
    layout = SeriesLayout(L, max(s.reach() for s in specs))
    flat, wf, bf = _params(blocks, gen)
    prepped = [_prep_params(flat[10 * l:10 * l + 10], s) for l, s in enumerate(specs)]
    bias_total = torch.stack([p[7] for p in prepped]).sum(0).contiguous() if training else None
    # an entry conv (k = 2, 11 -> C, with bias) and a 1x1 conv without bias, as the convs around the stack
    cw = [torch.nn.Parameter(torch.randn(C, 11, 2, generator=gen).to(DEV)), torch.nn.Parameter(torch.randn(MS, MS, 1, generator=gen).to(DEV))]
    cb = torch.nn.Parameter(torch.randn(C, generator=gen).to(DEV))
    convs = [(_lib.ConvShape(B, L, 11, C, 2, 1, 1, layout.ld, layout.halo), cw[0].detach(), cb.detach()),
             (_lib.ConvShape(B, L, MS, MS, 1, 1, 1, layout.ld, layout.halo), cw[1].detach(), None)]
    storages = StackPackTable.dynamic_storages(flat + [bias_total] + cw + [cb])
    assert storages is not None and len(storages) == (3 if training else 2)
    table = StackPackTable(lib, specs, B, layout, prepped, bias_total, convs, storages, DEV)
    assert table.njobs == 4 * len(blocks) + int(training) + 2 * len(convs)
    packed = table.run(lib, storages, DEV, out=torch.zeros(table.total, dtype=torch.uint8, device=DEV))
    _check_images(table, packed, *_reference_images(lib, specs, layout, prepped, bias_total, convs))

    # an in-place optimizer update of the parameters: the same table, launched again, packs the new weights ...
    with torch.no_grad():
        for t in flat + cw + [cb]:
            if isinstance(t, torch.nn.Parameter):
                t.add_(torch.randn(t.shape, generator=gen).to(DEV))
    # ... and so it does after the dynamic tensors have MOVED (new storages of the same sizes, other values, other addresses)
    keep = (wf, bf, bias_total)                                   # the old storages stay allocated: the new ones cannot reuse them
    wf2, bf2 = torch.randn(wf.shape, generator=gen).to(DEV), torch.randn(bf.shape, generator=gen).to(DEV)
    assert wf2.data_ptr() != wf.data_ptr() and bf2.data_ptr() != bf.data_ptr()
    flat2 = list(flat)
    for l in range(len(blocks)):
        flat2[10 * l + 6], flat2[10 * l + 7] = wf2[l], bf2[l]
    prepped2 = [_prep_params(flat2[10 * l:10 * l + 10], s) for l, s in enumerate(specs)]
    bias_total2 = torch.stack([p[7] for p in prepped2]).sum(0).contiguous() if training else None
    storages2 = StackPackTable.dynamic_storages(flat2 + [bias_total2] + cw + [cb])
    assert StackPackTable.key_of(specs, B, layout, prepped2, bias_total2, convs, storages2) == \
        StackPackTable.key_of(specs, B, layout, prepped, bias_total, convs, storages)          # the cached table still applies
    packed2 = table.run(lib, storages2, DEV, out=torch.zeros(table.total, dtype=torch.uint8, device=DEV))
    assert not torch.equal(packed2, packed)
    _check_images(table, packed2, *_reference_images(lib, specs, layout, prepped2, bias_total2, convs))
    del keep


def test_too_many_dynamic_storages_fall_back_to_per_object_packing():
    """plain tensors as parameters (every one its own storage): no table, and the stack still computes the same"""
    from wavenet_speech_amd.modules.wavenet import WaveNet
    torch.manual_seed(2)
    net = WaveNet(11, 2, STACKS["mixed_k2_k3"], MS, softmax=False).to(DEV)
    x = torch.randn(B, 11, 130, device=DEV)
    y = net(x)
    specs = [blk.spec(MS) for blk in net.convolutions]
    from wavenet_speech_amd.modules.block import fold_bottlenecks
    wfs, bfs = fold_bottlenecks(list(net.convolutions), list(net.bottlenecks))
    flat = []
    for blk, w, b in zip(net.convolutions, wfs, bfs):
        flat.extend(t.detach().clone() for t in blk.hip_params(w, b))
    assert StackPackTable.dynamic_storages(flat) is None
    cache = HF.PackCache()
    h = net.entry_conv1d(x)
    S = HF.residual_stack(h, specs, flat, pack_cache=cache)
    assert not cache.tables
    from wavenet_speech_amd.modules.pointwise import run_sequential
    assert torch.equal(run_sequential(net.output_stack, S), y.detach())
