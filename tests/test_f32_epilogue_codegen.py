"""CPU (hipcc cross-compiles without a GPU): the full-tile form of the fp32 series GEMM's EPI_DGATE epilogue keeps its memory
operations in flight -- checked on the gfx950 assembly, because the property is hipcc's to lose.

On this target `vmcnt` counts loads and stores together, in issue order.  The epilogue works in batches of rows: it issues the
next batch's loads of z and sigmoid (the look-ahead group), then consumes the current batch row by row and stores da and dg.  A
wait in front of a row must retire that row's loads and nothing younger: not a load of the look-ahead group it has just issued
(that would be no read-ahead at all) and not a store issued since the look-ahead group before it (that would put a write
acknowledgement on every batch's critical path).  With a branch around each row's stores hipcc cannot count the stores of the
skipped path and waits for too much; the full-tile form is straight-line code, and its counts are exact.

The test reads only waits, loads, stores and branches."""
import re
import subprocess

import pytest

from tools.listing import NO_HIPCC, listing

pytestmark = pytest.mark.skipif(NO_HIPCC, reason="hipcc not installed")

EPI_DGATE = 2
LOAD = re.compile(r"(global|buffer|flat)_load_")
STORE = re.compile(r"(global|buffer|flat)_store_")
WAIT = re.compile(r"s_waitcnt\b.*\bvmcnt\((\d+)\)")
BRANCH = re.compile(r"s_(c?branch|setpc|endpgm)")
LABEL = re.compile(r"[.\w$]+:")


def dgate_instantiations(text):
    """(MT, WPS, mangled name, instruction lines) of every series_gemm_kernel<MT, 4, EPI_DGATE, ...> in the listing"""
    out = []
    for m in re.finditer(r"^(_ZN2wn18series_gemm_kernel\w+):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S | re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        mt, nt, epi, _pfb, wps = [int(v) for v in re.search(r"series_gemm_kernel<(\d+), (\d+), (\d+), (\d+), (\d+)>", name).groups()]
        if nt == 4 and epi == EPI_DGATE:
            out.append((mt, wps, m.group(1), [l.strip() for l in m.group(2).splitlines() if l.strip() and not l.strip().startswith(";")]))
    return out


def straight_runs(lines):
    """the function cut at every label and after every branch: (index of the first line, lines) of each piece"""
    runs, cur, start = [], [], 0
    for i, l in enumerate(lines):
        if LABEL.match(l):
            if cur:
                runs.append((start, cur))
            cur, start = [], i + 1
            continue
        if not cur:
            start = i
        cur.append(l)
        if BRANCH.match(l):
            runs.append((start, cur))
            cur = []
    if cur:
        runs.append((start, cur))
    return runs


def full_tile_run(lines, mt):
    """the branch-free, label-free run after the K loop that holds the whole tile's 32 MT loads and 32 MT stores, or None.
    After the K loop in control flow -- hipcc is free to place the block anywhere in the listing: the run has no MFMA (every
    block of the K loop has), and the only stores of the kernel are the epilogue's."""
    for _start, run in straight_runs(lines):
        nl, ns = sum(1 for l in run if LOAD.match(l)), sum(1 for l in run if STORE.match(l))
        if nl == 32 * mt and ns == 32 * mt and not any(l.startswith("v_mfma") for l in run):
            return run
    return None


def early_retirements(run, mt):
    """simulate the in-order vmcnt queue over the run; the waits of the second batch to the last but one that retire a load of the
    most recent look-ahead group or a store issued since the look-ahead group before it, as (batch, count, what was retired)"""
    per_batch = 2 * (8 if mt == 4 else 4)         # z and sigmoid loads of a batch of rows; as many stores of da and dg
    nbatch = 32 * mt // per_batch
    queue, bad = [], []                           # queue entries: (kind, group or batch, position in the run)
    nload = nstore = 0
    first_pos = {}                                # look-ahead group -> position of its first load
    for pos, l in enumerate(run):
        if LOAD.match(l):
            g = nload // per_batch
            first_pos.setdefault(g, pos)
            queue.append(("load", g, pos))
            nload += 1
        elif STORE.match(l):
            queue.append(("store", nstore // per_batch, pos))
            nstore += 1
        else:
            w = WAIT.match(l)
            if not w:
                continue
            keep = int(w.group(1))
            retired, queue = (queue[:len(queue) - keep], queue[len(queue) - keep:]) if len(queue) > keep else ([], queue)
            batch = nstore // per_batch
            if not 1 <= batch <= nbatch - 2:
                continue
            recent = (nload - 1) // per_batch
            since = first_pos[recent - 1]
            early = [q for q in retired if (q[0] == "load" and q[1] == recent) or (q[0] == "store" and q[2] > since)]
            if early:
                bad.append((batch, keep, ["%s of batch %d" % q[:2] for q in early]))
    return bad


def resources(text, symbol):
    m = re.search(r"\.name:\s+%s\n(.*?)\.vgpr_count:\s+(\d+)" % re.escape(symbol), text, re.S)
    assert m, "no metadata for %s" % symbol
    # (.vgpr_count is the unified total on this target: 512 for the MT = 4 kernels, whose accumulators are AGPRs)
    return {"vgpr": int(m.group(2)), "private": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(1)).group(1))}


def failures(text):
    """what the listing of wn_gemm.hip violates, one line each; the number of instantiations looked at"""
    out, seen = [], 0
    for mt, wps, symbol, lines in dgate_instantiations(text):
        seen += 1
        what = "series_gemm_kernel<%d,4,2,..,%d>" % (mt, wps)
        run = full_tile_run(lines, mt)
        if run is None:
            out.append("%s: no straight-line run after the K loop with %d loads and %d stores" % (what, 32 * mt, 32 * mt))
        else:
            for batch, keep, early in early_retirements(run, mt):
                out.append("%s: batch %d: vmcnt(%d) retires %s" % (what, batch, keep, ", ".join(early)))
        res = resources(text, symbol)
        if res["private"] != 0:
            out.append("%s: %d bytes of scratch" % (what, res["private"]))
        if wps == 2 and res["vgpr"] > 256:
            out.append("%s: %d VGPRs do not fit two waves per SIMD" % (what, res["vgpr"]))
    return out, seen


def test_full_tile_dgate_epilogue_waits_for_exactly_its_rows():
    # MT = 1 and 2 at two waves per SIMD and MT = 4 at prefetch depth 3; the measurement build (csrc/wn_knobs.h) also holds MT = 4
    # at prefetch depth 1
    for defs, count in (("", 3), ("-DWN_MEASURE", 4)):
        bad, seen = failures(open(listing("wn_gemm.hip", defs=defs)).read())
        assert seen == count, (defs, seen)
        assert not bad, defs + "\n" + "\n".join(bad)


def test_the_rule_sees_a_wait_that_covers_the_previous_stores():
    """the rule on a hand-written run shaped like the ragged path's: per batch 8 look-ahead loads, then per row a wait and two
    stores.  vmcnt(22) in front of row 0 is exact (6 loads of its own batch, 8 stores of the batch before, 8 look-ahead loads);
    vmcnt(14) retires two of the previous batch's stores; a count below 8 reaches into the look-ahead group."""
    def run(first_wait):
        lines = ["global_load_dwordx4 v[0:3], v[4:5], off"] * 16
        for b in range(8):
            if 1 <= b < 7:
                lines += ["global_load_dwordx4 v[0:3], v[4:5], off"] * 8
            ahead = 8 if b < 7 else 0
            older_stores = 8 if b > 0 else 0
            for r in range(4):
                exact = (6 - 2 * r) + older_stores + ahead + 2 * r      # younger than row r's two loads
                lines += ["s_waitcnt vmcnt(%d)" % (first_wait if (b, r) == (3, 0) else exact)] + ["global_store_dwordx4 v[4:5], v[0:3], off"] * 2
        return lines
    assert early_retirements(run(22), 2) == []
    assert [b[:2] for b in early_retirements(run(14), 2)] == [(3, 14)]
    assert "store of batch 2" in early_retirements(run(14), 2)[0][2]
    assert "load of batch 4" in early_retirements(run(6), 2)[0][2]
