#!/usr/bin/env python3
"""Per row of scripts/register_bench.py (cloud, method, source order): the parent's runs, their spread, the branch's
runs and whether the branch's median lies inside the parent's own range.  Every run's figure is printed for wall_ms and
iter_ms; the other fields are counted in the last line alone.

  python profiles/r18/compare_register_bench.py DIR [RUNS]   (DIR holds rb_parent_K.jsonl and rb_branch_K.jsonl, K = 1..RUNS,
                                                              taken alternately; RUNS defaults to 3)
"""
import json
import os
import sys

import numpy as np

d = sys.argv[1]
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
FIELDS = ("wall_ms", "wall_one_iteration_ms", "iter_ms", "regularize_ms", "grid_ms")


def runs(side):
    out = {}
    for k in range(1, RUNS + 1):
        for line in open(os.path.join(d, f"rb_{side}_{k}.jsonl")):
            r = json.loads(line)
            out.setdefault((r["cloud"], r["method"], r["source_order"]), []).append(r)
    return out


P, B = runs("parent"), runs("branch")
outside = {f: 0 for f in FIELDS}
for key in P:
    same = all(b[f] == P[key][0][f] for b in B[key] + P[key] for f in ("iterations", "converged", "fitness", "error_to_truth"))
    print(f"{' '.join(key)}: results identical in every run: {same}")
    for f in FIELDS:
        p, b = [r[f] for r in P[key]], [r[f] for r in B[key]]
        med = float(np.median(b))
        inside = min(p) <= med <= max(p)
        outside[f] += not inside
        if f not in ("wall_ms", "iter_ms"):
            continue
        spread = (max(p) - min(p)) / np.median(p) * 100 if np.median(p) else 0.0
        print(f"  {f:>8}: parent {p} (spread {spread:.1f} %)  branch {b}  median {med:.4g} "
              f"{'inside' if inside else 'OUTSIDE (' + format((med / np.median(p) - 1) * 100, '+.1f') + ' % of the parent median)'}")
print("rows whose branch median lies outside the parent's range, of", len(P), ":", outside)
