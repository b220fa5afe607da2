#!/usr/bin/env python3
"""L2 counters per walking step of the XCD-local step pipeline, one row per dW1 pixel form, from the counters-only
passes of scripts/gpu_pmc_xstep_pix.sh (<dir>/pix<k>_counter_collection.csv): the plan of --steps steps is the
pipeline dispatch with the largest counters; its values are divided by --steps.

    python scripts/pmc_xstep_pix_table.py Outputs/pmc_xstep_pix [--steps 200]

FETCH-size counters are uncalibrated for this access pattern on gfx950: compare the rows' ratios, not the values."""
import argparse
import collections
import csv
import glob
import os
import re


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args(argv)
    rows = {}
    for p in sorted(glob.glob(os.path.join(a.dir, "**", "pix*_counter_collection.csv"), recursive=True)):
        form = re.search(r"(pix\d+)_counter_collection", p).group(1)
        disp = collections.defaultdict(lambda: collections.defaultdict(float))
        for r in csv.DictReader(open(p)):
            if "xstep_kernel" in r["Kernel_Name"]:
                disp[r["Dispatch_Id"]][r["Counter_Name"]] += float(r["Counter_Value"])
        if disp:
            rows[form] = max(disp.values(), key=lambda c: c.get("TCC_HIT_sum", 0.0) + c.get("TCC_MISS_sum", 0.0))
    names = sorted({c for v in rows.values() for c in v})
    print("| form | " + " | ".join(f"{c} / step" for c in names) + " | L2 hit |")
    print("|---|" + "---:|" * (len(names) + 1))
    for form, c in sorted(rows.items()):
        hit, miss = c.get("TCC_HIT_sum", 0.0), c.get("TCC_MISS_sum", 0.0)
        print(f"| {form} | " + " | ".join(f"{c.get(k, float('nan')) / a.steps:.0f}" for k in names) +
              f" | {100 * hit / max(1.0, hit + miss):.1f} % |")


if __name__ == "__main__":
    main()
