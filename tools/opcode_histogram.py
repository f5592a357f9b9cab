#!/usr/bin/env python3
"""Per-kernel, per-opcode instruction counts of csrc files (hipcc --cuda-device-only -S for gfx950): the mnemonic alone, no
registers, no order.  Two trees compare with `diff` of the two outputs; a refactor that leaves the code alone leaves them equal.

    tools/opcode_histogram.py [--csrc DIR] wn_pileup.hip ...      one line per kernel and opcode: file kernel opcode count
    tools/opcode_histogram.py --totals ...                        one line per kernel: file kernel instructions"""
import argparse, collections, os, re, subprocess, sys, tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--csrc", default=os.path.join(root, "wavenet_speech_amd", "csrc"))
ap.add_argument("--totals", action="store_true")
ap.add_argument("files", nargs="+")
args = ap.parse_args()
tmp = tempfile.mkdtemp(prefix="wn_ops_")
for f in args.files:
    out = os.path.join(tmp, f + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(args.csrc, f), "-o", out], check=True)
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(out).read(), re.M))
    cur, hist = None, collections.defaultdict(collections.Counter)
    for line in open(out):
        m = re.match(r"^(\w+):", line)
        if m:
            cur = m.group(1) if m.group(1) in kernels else cur
            continue
        if re.match(r"^\s*\.end_amdhsa_kernel|^\s*\.section", line):
            cur = None if line.lstrip().startswith(".section") else cur
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)(\s|$)", line)
        if cur and m and not line.lstrip().startswith("."):
            hist[cur][m.group(1)] += 1
    for k in sorted(hist):
        name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip().split("(")[0]
        if args.totals:
            print(f, name, sum(hist[k].values()))
        else:
            for op in sorted(hist[k]):
                print(f, name, op, hist[k][op])
