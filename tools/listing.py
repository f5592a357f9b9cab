"""What hipcc makes of one csrc file, by the flags of csrc/Makefile and nothing else: the `listing` and `remarks` targets there
add to the object rule's own command line what turns it into a device listing or into resource remarks.  No optimisation level,
language standard, architecture or per-file flag stands here."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wavenet_speech_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NO_HIPCC = not os.path.exists(HIPCC)            # the skipif condition of the codegen tests

compiles = 0                                    # runs of the compiler by this process
_DONE = {}


def _make(target, src, csrc, suffix, defs=""):
    """the path of what `target` makes of `csrc/src`, made at most once per process.  Another tree's files are compiled by
    this tree's Makefile, so both get the same flags; `defs` ("-DWN_MEASURE": the measurement build) is the Makefile's DEFS"""
    global compiles
    csrc = os.path.abspath(csrc or CSRC)
    key = (target, csrc, src) + ((defs,) if defs else ())
    if key in _DONE and os.path.exists(_DONE[key]):
        return _DONE[key]
    out = os.path.join(tempfile.mkdtemp(prefix="wn_%s_" % target), src + suffix)
    compiles += 1
    r = subprocess.run(["make", "-s", "-C", csrc, "-f", os.path.join(CSRC, "Makefile"), target, "SRC=" + src, "OUT=" + out, "HIPCC=" + HIPCC, "DEFS=" + defs],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError((r.stderr + (open(out).read() if target == "remarks" and os.path.exists(out) else ""))[-2000:])
    _DONE[key] = out
    return out


def listing(src, csrc=None, defs=""):
    """the path of the gfx950 assembly listing of csrc/<src>"""
    return _make("listing", src, csrc, ".s", defs)


def kernels(text):
    """[(symbol, .private_segment_fixed_size of its metadata)] of every .amdhsa_kernel of a listing, in the listing's order"""
    out = []
    for symbol in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        m = re.search(r"\.name:\s+%s\n.*?\.private_segment_fixed_size:\s*(\d+)" % re.escape(symbol), text, re.S)
        out.append((symbol, int(m.group(1)) if m else None))
    return out


def resources(src, csrc=None, defs=""):
    """one dict per kernel of csrc/<src> from hipcc's kernel-resource-usage remarks: "Function Name" and every remark row
    ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", ...) as strings"""
    rows, cur = [], None
    for line in open(_make("remarks", src, csrc, ".txt", defs)):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"Function Name": m.group(1)}
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w \[\]/]*): (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
            if m.group(1).startswith("LDS Size"):
                rows.append(cur)
                cur = None
    return rows
