#!/usr/bin/env python3
"""Per-kernel VALU wave instructions of ONE proof made under load, from two counter runs of tools/prof_loaded_proofs.py that differ
only in their rounds (bench.py's valu_under_load takes the same difference over all kernels): whatever the context's creation
launched cancels.
usage: python tools/pmc_per_proof.py A.json B.json PROOFS_BETWEEN      (A, B: tools/pmc_summary.py --json of the two runs)"""
import json
import sys

a, b = (json.load(open(p))["kernels"] for p in sys.argv[1:3])
proofs = float(sys.argv[3])
rows = []
for k in sorted(set(a) | set(b)):
    va = a.get(k, {}).get("counters", {}).get("SQ_INSTS_VALU", 0.0)
    vb = b.get(k, {}).get("counters", {}).get("SQ_INSTS_VALU", 0.0)
    rows.append((k, (vb - va) / proofs, (b.get(k, {}).get("calls", 0) - a.get(k, {}).get("calls", 0)) / proofs))
total = sum(r[1] for r in rows) or 1.0
print("%-56s %16s %8s %10s" % ("kernel", "SQ_INSTS_VALU/proof", "share", "calls/proof"))
for k, v, c in sorted(rows, key=lambda r: -r[1]):
    if v or c:
        print("%-56s %16.0f %7.1f%% %10.2f" % (k, v, 100 * v / total, c))
print("%-56s %16.0f" % ("wave_instructions_per_proof (all kernels)", total))
