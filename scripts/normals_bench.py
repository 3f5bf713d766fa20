#!/usr/bin/env python3
"""Device cost of normal and covariance estimation, one JSON line per cloud: fdm_cloud_estimate_normals
(normals and covariances in one pass) at k = 20 on device-resident clouds of the three sizes of BASELINE.json — the
28.8 K-point VLP-16 scan, the 272 K-point RGB-D frame and the 2.1 M-point 128-beam scan of fastdem_amd.synth, in the
world frame — and beside each fdm_statistical_outlier_removal's search on the same cloud with the same k: the fair
comparison for a search that also carries who the neighbours are (and whose lanes do the PCA).

ms = median over --repeat calls of the four device intervals fdm_normals_last_stats reports (grid build, search with
the fused PCA, fallback queue, what is left: the counters' read-back) — fdm_cloud_debug_profile switches the events on;
sor_* = the outlier removal's grid build, search and queue from fdm_sor_last_stats; wall_ms = the whole synchronous
call, allocations and events included.

  python scripts/normals_bench.py [--repeat 7] [--k 20] [--out profiles/normals/normals_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def world_cloud(F, name):
    """One scan of the synthetic workload as x, y, z float32 arrays in the world frame."""
    wl = F.synth.make(name, n_scans=1)
    s = wl.scan(0)
    T = np.asarray(wl.pose(0), dtype=np.float64).reshape(4, 4) @ np.asarray(wl.T_base_sensor, dtype=np.float64).reshape(4, 4)
    P = np.stack([s["x"], s["y"], s["z"]], axis=0).astype(np.float64)
    W = T[:3, :3] @ P + T[:3, 3:4]
    ok = np.isfinite(W).all(axis=0)
    return tuple(np.ascontiguousarray(W[a][ok], dtype=np.float32) for a in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--clouds", default="vlp16,rgbd,lidar128")
    args = ap.parse_args()
    import torch
    import fastdem_amd as F
    lib = F.capi.load()
    lib.fdm_cloud_debug_profile(1)
    lines = []
    for name in args.clouds.split(","):
        dev = [torch.from_numpy(v).cuda() for v in world_cloud(F, name)]
        n = int(dev[0].numel())
        F.estimate_normals(*dev, args.k, covariances=True)           # warm-up: code objects, the allocator
        F.statistical_outlier_removal(*dev, args.k)
        parts, wall, sor = [], [], []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, st = F.estimate_normals(*dev, args.k, covariances=True, return_stats=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            parts.append(st["ms"])
            F.statistical_outlier_removal(*dev, args.k)
            sor.append(F.sor_last_stats())
        med = np.median(np.asarray(parts), axis=0)
        sor_ms = np.median(np.asarray([s["ms"] for s in sor]), axis=0)
        line = {"cloud": name, "n": n, "k": args.k, "grid": [st["grid_x"], st["grid_y"]], "voxel": round(st["voxel"], 5),
                "n_fallback": st["n_fallback"], "n_invalid": st["n_invalid"],
                "grid_ms": round(float(med[0]), 4), "search_ms": round(float(med[1]), 4),
                "queue_ms": round(float(med[2]), 4), "write_ms": round(float(med[3]), 4),
                "ms": round(float(np.median(np.asarray(parts).sum(axis=1))), 4),
                "wall_ms": round(float(np.median(wall)), 3),
                "sor_n_fallback": sor[-1]["n_fallback"], "sor_grid_ms": round(float(sor_ms[0]), 4),
                "sor_search_ms": round(float(sor_ms[1]), 4), "sor_queue_ms": round(float(sor_ms[2]), 4)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
