"""Summarise scripts/pmc_memops.sh: per (solver, env count), the step kernel's executed instructions by
class per wave per launch (median over the step launches after the first two) and per physics substep.

    python scripts/pmc_memops_summary.py build/pmc_memops/pmcmem > build/pmc_memops/pmc_memops.json
"""
import csv
import glob
import json
import statistics
import sys

prefix = sys.argv[1]
SUBSTEPS = 20
out = {"note": __doc__.split("\n\n")[0].replace("\n", " ")}
for d in sorted(glob.glob(prefix + "_*")):
    if d.endswith(".log"):
        continue
    per = {}
    for fn in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
        for row in csv.DictReader(open(fn)):
            if "step_kernel" not in row["Kernel_Name"]:
                continue
            per.setdefault(row["Dispatch_Id"], {}).setdefault(row["Counter_Name"], 0.0)
            per[row["Dispatch_Id"]][row["Counter_Name"]] += float(row["Counter_Value"])
    ks = sorted(per, key=int)[2:]
    if not ks:
        continue
    v = {c: statistics.median(per[k][c] for k in ks) for c in per[ks[0]]}
    w = v.pop("SQ_WAVES")
    out[d[len(prefix) + 1:]] = {
        "launches": len(ks), "waves": w,
        "per_wave": {c.replace("SQ_INSTS_", ""): round(x / w, 1) for c, x in v.items()},
        "per_wave_substep": {c.replace("SQ_INSTS_", ""): round(x / w / SUBSTEPS, 1) for c, x in v.items()},
    }
print(json.dumps(out, indent=1))
