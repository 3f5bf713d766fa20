#!/usr/bin/env python3
"""Device cost of the cloud downsampling filters, one JSON line per measurement: fdm_cloud_voxel_grid in
its four modes and fdm_cloud_grid_max_z, at both orders, on device-resident clouds — the 272 K-point RGB-D frame (colour
channel) and the 2.1 M-point 128-beam scan (intensity channel) of fastdem_amd.synth — at 0.05 m and 0.2 m.

ms = median over --repeat calls of the three device intervals fdm_cloud_debug_last_ms reports (keys + sort, run heads +
staging, per-run reduction; fdm_cloud_debug_profile switches the events on) and their sum; wall_ms = the whole
synchronous call, allocations and those events included.

  python scripts/voxel_bench.py [--repeat 7] [--out profiles/voxel/voxel_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--clouds", default="rgbd,lidar128")
    args = ap.parse_args()
    import torch
    import fastdem_amd as F
    lib = F.capi.load()
    lib.fdm_cloud_debug_profile(1)

    def last_ms():
        ms = (C.c_float * 3)()
        lib.fdm_cloud_debug_last_ms(ms)
        return tuple(float(v) for v in ms)

    lines = []
    for name in args.clouds.split(","):
        s = F.synth.make(name, n_scans=1).scan(0)
        dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda()
               for k, v in s.items() if v is not None}
        kw = {k: dev[k] for k in ("intensity", "rgb") if k in dev}
        n = int(dev["x"].numel())
        for size in (0.05, 0.2):
            for mode in ("centroid", "nearest", "any", "center", "max_z"):
                for order in (0, 1):
                    def call():
                        if mode == "max_z":
                            return F.grid_max_z(dev["x"], dev["y"], dev["z"], size, order=order, **kw)
                        return F.voxel_grid(dev["x"], dev["y"], dev["z"], size, mode, order=order, **kw)
                    call()  # warm-up: code objects, the allocator
                    parts, wall = [], []
                    for _ in range(args.repeat):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        out = call()
                        wall.append((time.perf_counter() - t0) * 1e3)
                        parts.append(last_ms())
                    med = np.median(np.asarray(parts), axis=0)
                    line = {"cloud": name, "n": n, "channels": sorted(kw), "size": size, "mode": mode, "order": order,
                            "n_out": int(out["x"].numel()), "sort_ms": round(float(med[0]), 4),
                            "heads_ms": round(float(med[1]), 4), "reduce_ms": round(float(med[2]), 4),
                            "ms": round(float(np.median(np.asarray(parts).sum(axis=1))), 4),
                            "wall_ms": round(float(np.median(wall)), 3)}
                    lines.append(line)
                    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
