#!/usr/bin/env python3
"""Are the kernels of two builds of csrc the same code?  Every file of the Makefile's SRCS is compiled twice through
tools/listing.py (both by THIS tree's Makefile) and, for every kernel both listings hold, the instruction text from its label to
its end marker and its .amdhsa_ descriptor block are compared.  Local labels carry the function's index in the file, which moves
when a kernel before it leaves: the index is dropped (from the labels, from the loop comments that name them, and with it
the padding between a label and its comment) before comparing, nothing else is.
    compare_listings.py OTHER_CSRC                  that tree's files against this tree's, product flags
    compare_listings.py --defs=-DWN_MEASURE         this tree's product build against its measurement build
    compare_listings.py OTHER_CSRC --defs=...       that tree's product build against this tree's build with DEFS
Prints one row per file (kernels before, kernels after, equal or the symbols that differ) and the symbols only one side has;
exit status 1 if a shared kernel differs."""
import argparse
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import listing  # noqa: E402


def srcs():
    text = open(os.path.join(listing.CSRC, "Makefile")).read()
    return re.search(r"^SRCS\s*:=\s*(.*)$", text, re.M).group(1).split()


def kernel_texts(path):
    """{symbol: (instruction text, descriptor block)} of a listing"""
    text = re.sub(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b", r".L\1\2", open(path).read())
    text = re.sub(r"\bBB\d+(_\d+)\b", r"BB\1", text)                # the same labels in the loop comments
    text = re.sub(r"[ \t]+;", " ;", text)                            # the padding in front of a comment follows the label's width
    out = {}
    for symbol, _ in listing.kernels(text):
        body = re.search(r"^%s:.*?^\.Lfunc_end:" % re.escape(symbol), text, re.S | re.M)
        desc = re.search(r"^\s*\.amdhsa_kernel\s+%s\n.*?\.end_amdhsa_kernel" % re.escape(symbol), text, re.S | re.M)
        out[symbol] = (body.group(0), desc.group(0))
    return out


def demangle(symbols):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not symbols or not tool:
        return list(symbols)
    return subprocess.run([tool] + list(symbols), capture_output=True, text=True, check=True).stdout.split("\n")[:len(symbols)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other_csrc", nargs="?", default=None)
    ap.add_argument("--defs", default="")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    files = srcs()
    with ThreadPoolExecutor(args.jobs) as pool:
        before = list(pool.map(lambda f: kernel_texts(listing.listing(f, args.other_csrc)), files))
        after = list(pool.map(lambda f: kernel_texts(listing.listing(f, None, args.defs)), files))
    bad = 0
    print("| file | kernels before | kernels after | shared kernels |")
    print("|---|---|---|---|")
    gone, new = [], []
    for f, b, a in zip(files, before, after):
        differ = [s for s in b if s in a and b[s] != a[s]]
        bad += len(differ)
        gone += [s for s in b if s not in a]
        new += [s for s in a if s not in b]
        print("| `%s` | %d | %d | %s |" % (f, len(b), len(a), "equal" if not differ else "DIFFER: " + ", ".join(demangle(differ))))
    for title, syms in (("only before", gone), ("only after", new)):
        print("%s: %d" % (title, len(syms)))
        for name in demangle(syms):
            print("    " + name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
