"""CPU: what the host side of libwavenet_amd.so answers without a GPU -- the profiler's kernel-class table, every size / plan
query and both pack-table builders over a fixed list of shapes, and the return codes of the four shape checks -- is held to
tests/golden/host_plans.json, which `collect()` below produced from the library of the commit named in its "source" field.  The
planning code is shared by many entry points; a refactor of it must leave every one of these numbers where it was."""
import ctypes
import hashlib
import json
import os

import pytest

from wavenet_speech_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_plans.json")
B = 2

KERNEL_NAMES = [
    "pack_kernel", "series_gemm_kernel<gate>", "series_gemm_kernel<res>", "series_gemm_kernel<dz,dgate>",
    "series_gemm_kernel<dx>", "wgrad_kernel", "wgrad_reduce_kernel", "series_gemm_kernel<conv_fwd>",
    "series_gemm_kernel<conv_bwd_data>", "series_gemm_kernel<skips_sum>", "hload_kernel", "hgemm_kernel<gate>",
    "hgemm_kernel<res>", "hgemm_kernel<dz,dgate>", "hgemm_kernel<dx>", "hgemm_kernel<skips_sum>", "hwgrad_kernel",
    "embed_kernel", "synth_kernel", "ctc_kernel", "hfused_fwd_kernel",
    "hgemm_kernel<conv_fwd>", "hgemm_kernel<conv_bwd_data>", "hcol_kernel<dz,dgate>", "hcol_kernel<dx>", "hcol2_kernel<dx+dz>",
    "hcol_kernel<skips_sum>"]

# (Ci, Co, Ms, k, L): each the smallest that reaches a branch of the half-precision block plan
HALF_BLOCKS = [
    (8, 8, 8, 2, 100),
    (64, 64, 64, 2, 96), (128, 128, 128, 2, 96),      # fused forward and column-owner backward
    (128, 128, 64, 2, 96),                            # fused, not column-owner
    (192, 192, 192, 2, 96),                           # the four-wave form in the one-plane modes
    (256, 256, 256, 2, 100), (256, 256, 256, 2, 128), (256, 256, 256, 2, 256),   # neither / narrow / wide 16x16x32 form in f16x3
    (64, 64, 64, 3, 96),                              # three taps: not fused
]
F32_BLOCKS = [(c, c, c, 2, 100) for c in (8, 64, 96, 256)] + [(64, 64, 64, 3, 96)]      # 1, 2, 3 and 8 row tiles; three taps
CONVS = [(64, 64, 1), (256, 256, 3)]                  # (Ci, Co, k): a 1x1 conv and a 3-tap conv
GEOMETRY = [(causal, d) for causal in (1, 0) for d in (1, 4)]
HALF_PRECISIONS = ("f16x3", "f16", "bf16")
STACKS = (3, 33)                                      # 33 blocks: more than one skips_sum group (WN_MAX_STACK_GROUP = 32)
KNOBS = (None, "WN_FUSED_FWD", "WN_COL_BWD", "WN_HWGRAD_COMPOSITE", "WN_COL_PAIR")      # the ones read per call, each set to 0


def _reach(k, d, causal):
    return max(abs(o) for o in _lib.tap_offsets(k, d, causal))


def _params(n, first=0x100000):
    """n blocks' parameter structs of made-up, non-null addresses (nothing is dereferenced on the host); the skip biases are
    equally spaced, as the half builder requires of a stacked tensor"""
    out = []
    for l in range(n):
        base = first + l * 0x10000
        vals = [base + 0x1000 * i for i in range(10)]
        vals[7] = first + 0x4000000 + 0x400 * l           # b_skip
        out.append(_lib.BlockParams(*vals))
    return (_lib.BlockParams * n)(*out)


def _block_shape(case, causal, d, layout):
    ci, co, ms, k, L = case
    ld, halo = layout(L, _reach(k, d, causal))
    return _lib.BlockShape(B, L, ci, co, ms, k, d, causal, ld, halo)


def _skipsum_shape(sh, n):
    ss = _lib.SkipSumShape(sh.batch, sh.length, sh.skip_rows, n, sh.ld, sh.halo)
    for i in range(n):
        ss.channels[i] = sh.out_channels
    return ss


def _ramp(offsets):
    """the offsets of equal blocks are equally spaced: written as [first, step, count] (nothing is lost), or as they are"""
    steps = {b - a for a, b in zip(offsets, offsets[1:])}
    return dict(first=offsets[0], step=steps.pop(), count=len(offsets)) if len(offsets) > 2 and len(steps) == 1 else list(offsets)


def stack_table(lib, sh, n, with_skipsum, convs=()):
    """wn_stack_pack_table_build for n blocks of shape sh (+ convs in the same layout) -> (scalars, raw table bytes)"""
    shapes = (_lib.BlockShape * n)(*([sh] * n))
    carr = (_lib.PackConv * max(1, len(convs)))(*[_lib.PackConv(c, 0x9000000 + 0x100000 * i, 0x9800000 + 0x1000 * i)
                                                  for i, c in enumerate(convs)])
    dyn = (_lib.MemRange * 1)(_lib.MemRange(0x100000, 0))
    nbytes = lib.wn_stack_pack_table_bytes(n, len(convs))
    host = ctypes.create_string_buffer(max(1, nbytes))
    offs, soffs, coffs = (ctypes.c_size_t * n)(), (ctypes.c_size_t * 2)(), (ctypes.c_size_t * max(1, len(convs)))()
    total, njobs, nblk = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.wn_stack_pack_table_build(shapes, _params(n), n, with_skipsum, 0x8000000 if with_skipsum else None, carr, len(convs),
                                       dyn, 0, host, nbytes, offs, soffs, coffs, ctypes.byref(total), ctypes.byref(njobs),
                                       ctypes.byref(nblk))
    ngroups = (n + _lib.MAX_STACK_GROUP - 1) // _lib.MAX_STACK_GROUP if with_skipsum else 0
    res = dict(rc=rc, bytes=nbytes, blocks=_ramp(list(offs)), skipsum=list(soffs)[:ngroups], convs=list(coffs)[:len(convs)],
               total=total.value, njobs=njobs.value, launch_blocks=nblk.value)
    return res, host.raw


def hstack_table(lib, sh, prec, n, with_skipsum):
    """wn_hstack_pack_table_build for n blocks of shape sh -> (scalars, raw table bytes)"""
    shapes = (_lib.BlockShape * n)(*([sh] * n))
    dyn = (_lib.MemRange * 1)(_lib.MemRange(0x100000, 0))
    nbytes = lib.wn_hstack_pack_table_bytes(n)
    host = ctypes.create_string_buffer(max(1, nbytes))
    offs, soffs = (ctypes.c_size_t * n)(), (ctypes.c_size_t * 2)()
    total, njobs, nblk = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.wn_hstack_pack_table_build(shapes, _params(n), n, prec, with_skipsum, dyn, 0, host, nbytes, offs, soffs,
                                        ctypes.byref(total), ctypes.byref(njobs), ctypes.byref(nblk))
    ngroups = (n + _lib.MAX_STACK_GROUP - 1) // _lib.MAX_STACK_GROUP if with_skipsum else 0
    res = dict(rc=rc, bytes=nbytes, blocks=_ramp(list(offs)), skipsum=list(soffs)[:ngroups], total=total.value, njobs=njobs.value,
               launch_blocks=nblk.value)
    return res, host.raw


def _dims(case):
    return "x".join(map(str, case))


def _off(knob):
    return " %s=0" % knob if knob else ""


def f32_cases():
    for case in F32_BLOCKS:
        for causal, d in GEOMETRY:
            yield "f32 %s causal=%d d=%d" % (_dims(case), causal, d), case, causal, d


def half_cases():
    for knob in KNOBS:
        for case in HALF_BLOCKS:
            for causal, d in GEOMETRY:
                for pname in HALF_PRECISIONS:
                    yield "%s %s causal=%d d=%d%s" % (pname, _dims(case), causal, d, _off(knob)), case, causal, d, pname, knob


class knob_off:
    """os.environ[knob] = "0" for the block, then the environment as it was (the library reads these per call)"""
    def __init__(self, knob):
        self.knob = knob

    def __enter__(self):
        if self.knob:
            self.old = os.environ.get(self.knob)
            os.environ[self.knob] = "0"

    def __exit__(self, *exc):
        if self.knob:
            if self.old is None:
                del os.environ[self.knob]
            else:
                os.environ[self.knob] = self.old


def conv_shapes(layout, causal=1):
    out = []
    for ci, co, k in CONVS:
        ld, halo = layout(100, _reach(k, 1, causal))
        out.append(_lib.ConvShape(B, 100, ci, co, k, 1, causal, ld, halo))
    return out


def collect_plans(lib):
    ref = ctypes.byref
    out = {}
    for L, reach in ((100, 0), (100, 3), (128, 8), (16000, 512)):
        out["layout %d %d" % (L, reach)] = dict(series=list(_lib.series_layout(L, reach)), hseries=list(_lib.hseries_layout(L, reach)))
    for name, case, causal, d in f32_cases():
        sh = _block_shape(case, causal, d, _lib.series_layout)
        e = dict(ld=sh.ld, halo=sh.halo, packed=lib.wn_block_packed_bytes(ref(sh)), wgrad_ws=lib.wn_block_wgrad_workspace_bytes(ref(sh)))
        # the convs of a stack share its layout: theirs reach further than a dilation-1 block's taps, so take the wider one
        ld, halo = _lib.series_layout(case[4], max(_reach(case[3], d, causal), 2))
        shc = _lib.BlockShape(B, case[4], case[0], case[1], case[2], case[3], d, causal, ld, halo)
        convs = [_lib.ConvShape(B, case[4], ci, co, k, 1, causal, ld, halo) for ci, co, k in CONVS]
        for n in STACKS:
            e["skipsum_packed %d" % n] = lib.wn_skipsum_packed_bytes(ref(_skipsum_shape(sh, min(n, _lib.MAX_STACK_GROUP))))
            for ws in (0, 1):
                e["table %d skipsum=%d" % (n, ws)] = stack_table(lib, sh, n, ws)[0]
                e["table %d skipsum=%d convs" % (n, ws)] = stack_table(lib, shc, n, ws, convs)[0]
        out[name] = e
    for name, case, causal, d, pname, knob in half_cases():
        prec = _lib.PRECISIONS[pname]
        with knob_off(knob):
            sh = _block_shape(case, causal, d, _lib.hseries_layout)
            three = (_lib.BlockShape * 3)(sh, sh, sh)
            e = dict(ld=sh.ld, halo=sh.halo,
                     series_bytes=lib.wn_hseries_bytes(prec, B, case[0], sh.ld),
                     packed=lib.wn_hblock_packed_bytes(ref(sh), prec),
                     fused=lib.wn_hblock_forward_is_fused(ref(sh), prec),
                     pair_fused=lib.wn_hblock_backward_pair_is_fused(ref(sh), ref(sh), prec),
                     wgrad_ws=lib.wn_hblock_wgrad_workspace_bytes(ref(sh), prec),
                     group_max=lib.wn_hblocks_wgrad_group_max(ref(sh), prec),
                     group_ws=lib.wn_hblocks_wgrad_workspace_bytes(three, 3, prec))
            for n in STACKS:
                e["skipsum_packed %d" % n] = lib.wn_hskipsum_packed_bytes(ref(_skipsum_shape(sh, min(n, _lib.MAX_STACK_GROUP))), prec)
                for ws in (0, 1):
                    e["table %d skipsum=%d" % (n, ws)] = hstack_table(lib, sh, prec, n, ws)[0]
        out[name] = e
    for knob in KNOBS:
        with knob_off(knob):
            for causal in (1, 0):
                for i, (cf, ch) in enumerate(zip(conv_shapes(_lib.series_layout, causal), conv_shapes(_lib.hseries_layout, causal))):
                    e = dict(packed=lib.wn_conv_packed_bytes(ref(cf)), wgrad_ws=lib.wn_conv_wgrad_workspace_bytes(ref(cf)))
                    for pname in HALF_PRECISIONS:
                        prec = _lib.PRECISIONS[pname]
                        e["%s packed" % pname] = lib.wn_hconv_packed_bytes(ref(ch), prec)
                        e["%s wgrad_ws" % pname] = lib.wn_hconv_wgrad_workspace_bytes(ref(ch), prec)
                    out["conv %s causal=%d%s" % (_dims(CONVS[i]), causal, _off(knob))] = e
    return out


def collect_errors(lib):
    """return codes of one entry point behind each of check_block / check_conv / check_hblock / check_hconv, every other pointer
    NULL (so a shape that passes answers WN_ERR_NULL = -3)"""
    ref = ctypes.byref

    def block(layout, **kw):
        f = dict(batch=B, length=100, in_channels=8, out_channels=8, skip_rows=8, kernel_width=2, dilation=4, causal=1)
        f["ld"], f["halo"] = layout(100, 4)
        f.update(kw)
        return _lib.BlockShape(*[f[n] for n, _ in _lib.BlockShape._fields_])

    def conv(layout, **kw):
        f = dict(batch=B, length=100, in_channels=8, out_channels=8, kernel_width=2, dilation=4, causal=1)
        f["ld"], f["halo"] = layout(100, 4)
        f.update(kw)
        return _lib.ConvShape(*[f[n] for n, _ in _lib.ConvShape._fields_])

    bad = {"ok": {}, "zero channels": dict(in_channels=0), "zero out channels": dict(out_channels=0), "kernel_width 0": dict(kernel_width=0),
           "kernel_width 9": dict(kernel_width=9, dilation=1), "channels 1025": dict(in_channels=1025),
           "out channels 1025": dict(out_channels=1025), "zero dilation": dict(dilation=0),
           "halo below reach": dict(dilation=16),                                    # taps reach 16, the halo is 4 (fp32) / 8 (half)
           "kernel_width 9 and zero channels": dict(kernel_width=9, in_channels=0),   # BAD_SHAPE comes before UNSUPPORTED
           "channels 1025 and halo below reach": dict(in_channels=1025, dilation=16)}
    out = {}
    f16 = _lib.PRECISIONS["f16"]
    calls = {
        "wn_block_forward": lambda s: lib.wn_block_forward(s, None, None, None, None, 0, None, None, None),
        "wn_conv_forward": lambda s: lib.wn_conv_forward(s, None, None, None, None),
        "wn_hblock_forward": lambda s, p=f16: lib.wn_hblock_forward(s, p, None, None, None, None, 0, None, None, None, None),
        "wn_hconv_forward": lambda s, p=f16: lib.wn_hconv_forward(s, p, None, None, None, None),
    }
    for fn, call in calls.items():
        half = fn.startswith("wn_h")
        layout = _lib.hseries_layout if half else _lib.series_layout
        make = block if "block" in fn else conv
        e = {"NULL shape": call(None)}
        for what, kw in bad.items():
            e[what] = call(ref(make(layout, **kw)))
        if "block" in fn:
            e["zero skip rows"] = call(ref(make(layout, skip_rows=0)))
            e["skip rows 1025"] = call(ref(make(layout, skip_rows=1025)))
        if half:
            for p in (0, 7):                            # f32 and a value that is no precision
                e["precision %d" % p] = call(ref(make(layout)), p)
                e["precision %d, NULL shape" % p] = call(None, p)                       # NULL comes first
                e["precision %d, zero channels" % p] = call(ref(make(layout, in_channels=0)), p)   # the precision before the shape
        out[fn] = e
    return out


def pack_plans(plans):
    """the golden's form of collect_plans()'s dict: many cases give the same answers, so each distinct answer is written once
    ("values") and every case, in the order collect_plans() makes them, names its answer by position ("index")"""
    values, index = [], []
    for v in plans.values():
        if v not in values:
            values.append(v)
        index.append(values.index(v))
    return dict(values=values, index=index, names_sha256=hashlib.sha256("\n".join(plans).encode()).hexdigest())


def unpack_plans(packed, names):
    assert len(names) == len(packed["index"]) and hashlib.sha256("\n".join(names).encode()).hexdigest() == packed["names_sha256"]
    return {n: packed["values"][i] for n, i in zip(names, packed["index"])}


def collect(lib):
    return dict(plans=pack_plans(collect_plans(lib)), errors=collect_errors(lib))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plans(golden):
    """(what this library answers, what the golden holds), both {case name: answers}"""
    before = dict(os.environ)
    got = collect_plans(_lib.load())
    assert dict(os.environ) == before
    return got, unpack_plans(golden["plans"], list(got))


def test_kernel_class_table():
    lib = _lib.load()
    assert lib.wn_prof_num_kernels() == 27 == len(KERNEL_NAMES)
    assert [lib.wn_prof_kernel_name(i).decode() for i in range(27)] == KERNEL_NAMES
    for i in (-1, 27, 1000):
        assert lib.wn_prof_kernel_name(i) == b""


def test_plans_match_the_golden(plans):
    got, want = plans
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, "%d of %d cases differ, the first: %s\n got  %r\n want %r" % (len(wrong), len(want), wrong[0], got[wrong[0]],
                                                                                   want[wrong[0]])


def test_the_cases_reach_the_plan_branches(plans):
    """the list above is only worth holding if it does reach the forms it names"""
    p = plans[1]
    at = lambda pname, case, knob=None: p["%s %s causal=1 d=1%s" % (pname, _dims(case), _off(knob))]
    assert at("f16", (64, 64, 64, 2, 96))["fused"] == 1 and at("f16", (64, 64, 64, 2, 96))["pair_fused"] == 1
    assert at("f16", (128, 128, 64, 2, 96))["fused"] == 1 and at("f16", (128, 128, 64, 2, 96))["pair_fused"] == 0
    assert at("f16x3", (64, 64, 64, 2, 96))["fused"] == 0 and at("f16", (64, 64, 64, 3, 96))["fused"] == 0
    assert at("f16", (64, 64, 64, 2, 96), "WN_FUSED_FWD")["fused"] == 0
    assert at("f16", (64, 64, 64, 2, 96), "WN_COL_BWD")["pair_fused"] == 0 and at("f16", (64, 64, 64, 2, 96), "WN_COL_PAIR")["pair_fused"] == 0
    assert at("f16", (64, 64, 64, 2, 96))["group_max"] > 1 and at("f16", (64, 64, 64, 2, 96), "WN_HWGRAD_COMPOSITE")["group_max"] == 1
    sizes = {L: at("f16x3", (256, 256, 256, 2, L))["packed"] for L in (100, 128, 256)}
    assert all(v > 0 for v in sizes.values())
    assert at("f16", (192, 192, 192, 2, 96))["packed"] > 0 and at("f16", (8, 8, 8, 2, 100))["table 33 skipsum=1"]["rc"] == 0
    assert len(at("f16", (8, 8, 8, 2, 100))["table 33 skipsum=1"]["skipsum"]) == 2


def test_shape_check_codes_match_the_golden(golden):
    got = collect_errors(_lib.load())
    assert got == golden["errors"]
    for fn, e in got.items():                       # and the golden itself says what include/wavenet_amd.h says
        assert e["ok"] == -3 and e["NULL shape"] == -3, fn
        assert e["zero channels"] == e["kernel_width 0"] == e["halo below reach"] == e["kernel_width 9 and zero channels"] == -1, fn
        assert e["kernel_width 9"] == e["channels 1025"] == e["channels 1025 and halo below reach"] == -2, fn
        if fn.startswith("wn_h"):
            assert e["precision 0"] == e["precision 7"] == e["precision 0, zero channels"] == -2 and e["precision 7, NULL shape"] == -3, fn
