"""CPU: the fp32 stack pack table (wn_stack_pack_table_build is host-only) lays the images out back to back -- each block's at the
size wn_block_packed_bytes gives, the long-K skips_sum weights at wn_skipsum_packed_bytes, the convs at wn_conv_packed_bytes."""
import ctypes

import pytest

from wavenet_speech_amd import _lib

C, MS, B = 40, 24, 2        # 40 channels: a ragged 32-row tile and cp8 padding; skip / out dim 24


def _layout(L, reach):
    return _lib.series_layout(L, reach)


def _build(lib, blocks, L, with_skipsum, convs, ndyn=0):
    """blocks: [(ci, co, k, d)]; convs: [(ci, co, k)].  Pointers are made-up addresses: nothing is dereferenced on the host."""
    reach = max([(k - 1) * d for _, _, k, d in blocks] + [k - 1 for _, _, k in convs] + [0])
    ld, halo = _layout(L, reach)
    n, nc = len(blocks), len(convs)
    shapes = (_lib.BlockShape * max(1, n))(*[_lib.BlockShape(B, L, ci, co, MS, k, d, 1, ld, halo) for ci, co, k, d in blocks])
    fake = iter(range(0x10000, 0x10000000, 0x10000))
    params = (_lib.BlockParams * max(1, n))(*[_lib.BlockParams(*[next(fake) for _ in range(10)]) for _ in blocks])
    cshapes = [_lib.ConvShape(B, L, ci, co, k, 1, 1, ld, halo) for ci, co, k in convs]
    carr = (_lib.PackConv * max(1, nc))(*[_lib.PackConv(sh, next(fake), next(fake)) for sh in cshapes])
    dyn = (_lib.MemRange * 1)(_lib.MemRange(0x10000, 0x100000 if ndyn else 0))
    nbytes = lib.wn_stack_pack_table_bytes(n, nc)
    host = ctypes.create_string_buffer(max(1, nbytes))
    offs = (ctypes.c_size_t * max(1, n))()
    soffs = (ctypes.c_size_t * max(1, (n + _lib.MAX_STACK_GROUP - 1) // _lib.MAX_STACK_GROUP))()
    coffs = (ctypes.c_size_t * max(1, nc))()
    total, njobs, nblk = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.wn_stack_pack_table_build(shapes, params, n, int(with_skipsum), next(fake) if with_skipsum else None, carr, nc, dyn, ndyn,
                                       host, nbytes, offs, soffs, coffs, ctypes.byref(total), ctypes.byref(njobs), ctypes.byref(nblk))
    return rc, dict(shapes=list(shapes)[:n], cshapes=cshapes, offs=list(offs)[:n], soffs=list(soffs), coffs=list(coffs)[:nc],
                    total=total.value, njobs=njobs.value, launch_blocks=nblk.value, table_bytes=nbytes, ld=ld, halo=halo)


STACKS = {
    "three_k2": [(C, C, 2, 1), (C, C, 2, 2), (C, C, 2, 4)],
    "one_k3": [(C, C, 3, 2)],
    "mixed": [(C, C, 2, 1), (C, C, 3, 2), (C, C, 2, 4)],
}


@pytest.mark.parametrize("L", [130, 128, 5])
@pytest.mark.parametrize("stack", sorted(STACKS))
@pytest.mark.parametrize("with_skipsum", [0, 1])
def test_offsets_and_sizes_follow_the_per_object_queries(stack, L, with_skipsum):
    lib = _lib.load()
    blocks = STACKS[stack]
    convs = [(11, C, 2), (MS, MS, 1), (MS, MS, 1)]            # an entry conv and the two 1x1 convs of an output block
    rc, t = _build(lib, blocks, L, with_skipsum, convs, ndyn=1)
    assert rc == 0
    want, at = [], 0
    for sh in t["shapes"]:
        size = lib.wn_block_packed_bytes(ctypes.byref(sh))
        assert size > 0 and size % 256 == 0
        want.append(at)
        at += size
    assert t["offs"] == want
    if with_skipsum:
        ss = _lib.SkipSumShape(B, L, MS, len(blocks), t["ld"], t["halo"])
        for i, (_ci, co, _k, _d) in enumerate(blocks):
            ss.channels[i] = co
        assert t["soffs"][0] == at
        at += lib.wn_skipsum_packed_bytes(ctypes.byref(ss))
    cwant = []
    for sh in t["cshapes"]:
        cwant.append(at)
        at += lib.wn_conv_packed_bytes(ctypes.byref(sh))
    assert t["coffs"] == cwant
    assert t["total"] == at
    assert t["njobs"] == 4 * len(blocks) + with_skipsum + 2 * len(convs)
    assert t["launch_blocks"] > 0
    per_job = lib.wn_stack_pack_table_bytes(1, 0) // 5        # one block alone: four arrangements and room for its skips_sum job
    assert t["table_bytes"] == per_job * (4 * len(blocks) + 1 + 2 * len(convs))


def test_convs_alone_and_bad_arguments():
    lib = _lib.load()
    rc, t = _build(lib, [], 130, 0, [(MS, MS, 1)])
    assert rc == 0 and t["coffs"] == [0] and t["njobs"] == 2
    sh = t["cshapes"][0]
    assert t["total"] == lib.wn_conv_packed_bytes(ctypes.byref(sh))
    assert lib.wn_stack_pack_table_bytes(0, 0) == 0
    rc, _ = _build(lib, [(C, C, 9, 1)], 130, 0, [])            # kernel_width 9 > WN_MAX_TAPS
    assert rc == -2
    assert lib.wn_stack_pack_run(None, 1, 1, None, 0, None, None) == -3
    assert lib.wn_stack_pack_run(None, 0, 0, None, 0, None, None) == -1
