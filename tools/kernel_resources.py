#!/usr/bin/env python3
"""Print VGPR/AGPR/spill/LDS/occupancy per kernel (hipcc -Rpass-analysis=kernel-resource-usage), of the product's code: the
command line is csrc/Makefile's (tools/listing.py)."""
import subprocess, sys
from listing import resources
for f in sys.argv[1:] or ["wn_gemm.hip", "wn_wgrad.hip", "wn_pack.hip"]:
    for cur in resources(f):
        name = subprocess.run(["c++filt", cur["Function Name"]], capture_output=True, text=True).stdout.strip()[:70]
        print("%-72s VGPR %4s AGPR %4s SGPR %4s spill %s/%s scratch %s LDS %6s occ %s" % (
            name, cur.get("VGPRs"), cur.get("AGPRs"), cur.get("TotalSGPRs"), cur.get("VGPRs Spill"),
            cur.get("SGPRs Spill"), cur.get("ScratchSize [bytes/lane]"), cur.get("LDS Size [bytes/block]"),
            cur.get("Occupancy [waves/SIMD]")))
