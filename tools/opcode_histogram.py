#!/usr/bin/env python3
"""Per-kernel, per-opcode instruction counts of csrc files (the device listing of tools/listing.py): the mnemonic alone, no
registers, no order.  Two trees compare with `diff` of the two outputs; a refactor that leaves the code alone leaves them equal.
The listing is made with the flags of this tree's csrc/Makefile, the per-file ones included, so the counts are of the product's
code.  Before the flags moved there this tool left the per-file flags out: its counts of wn_half.hip, wn_fused.hip and the four
wn_col*.hip files differ from those of earlier versions; every other file's are the same.

    tools/opcode_histogram.py [--csrc DIR] wn_pileup.hip ...      one line per kernel and opcode: file kernel opcode count
    tools/opcode_histogram.py --totals ...                        one line per kernel: file kernel instructions"""
import argparse, collections, re, subprocess

import listing

ap = argparse.ArgumentParser()
ap.add_argument("--csrc", default=listing.CSRC)
ap.add_argument("--totals", action="store_true")
ap.add_argument("files", nargs="+")
args = ap.parse_args()
for f in args.files:
    out = listing.listing(f, args.csrc)
    kernels = {k for k, _ in listing.kernels(open(out).read())}
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
