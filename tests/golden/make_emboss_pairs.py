#!/usr/bin/env python3
"""
Write tests/golden/emboss_pairs.json: the (true, predicted) base strings that the REFERENCE's evaluation notebook,
ipynbs/'RawCTCNet@AvgCTCLoss=0.6 Gaussian Model (Eval).ipynb', aligned with EMBOSS needle (EDNAFULL, gap open 10, gap extend
0.5, end gaps not penalised), with the Score / Identity / Gaps lines needle printed for them -- recorded results, data only.

Like make_golden.py this reads the reference (WN_REFERENCE, default /root/reference) and copies none of its code.  The
notebook records the pairs in two shapes: code cells with a '# ground truth: ...' comment whose output is the predicted
string, followed by a markdown cell with needle's report; and markdown cells with 'TRUE: ... PRED: ...' blocks and the report.
"""
import json
import os
import re

REF = os.environ.get("WN_REFERENCE", "/root/reference")
NOTEBOOK = os.path.join(REF, "ipynbs", "RawCTCNet@AvgCTCLoss=0.6 Gaussian Model (Eval).ipynb")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emboss_pairs.json")


def text(cell):
    return "".join(cell["source"])


def record(true, pred, report):
    score = float(re.search(r"# Score: ([\d.]+)", report).group(1))
    ident, length = re.search(r"# Identity:\s+(\d+)/(\d+)", report).groups()
    gaps, glen = re.search(r"# Gaps:\s+(\d+)/(\d+)", report).groups()
    assert length == glen
    return {"true": true, "pred": pred, "score": score, "identity": int(ident), "length": int(length), "gaps": int(gaps)}


def main():
    cells = json.load(open(NOTEBOOK))["cells"]
    pairs = []
    for n, cell in enumerate(cells):
        src = text(cell)
        truth = re.search(r"# ground truth: (\w+)", src)
        if truth and cell["cell_type"] == "code" and cell.get("outputs"):
            shown = "".join(line for out in cell["outputs"] for line in out.get("data", {}).get("text/plain", []))
            pairs.append(record(truth.group(1), shown.strip().strip("'"), text(cells[n + 1])))
    for cell in cells:
        src = text(cell)
        if "TRUE:" in src:
            for block in src.split("TRUE: ")[1:]:
                pairs.append(record(block.split("\n")[0].strip(), re.search(r"PRED: (\w+)", block).group(1), block))
    assert len(pairs) == 12, len(pairs)
    doc = {"source": "paultsw/wavenet-speech, ipynbs/RawCTCNet@AvgCTCLoss=0.6 Gaussian Model (Eval).ipynb",
           "tool": "EMBOSS needle, EDNAFULL (5 / -4), gap open 10, gap extend 0.5, end gaps not penalised",
           "pairs": pairs}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", OUT, len(pairs), "pairs")


if __name__ == "__main__":
    main()
