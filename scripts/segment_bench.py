#!/usr/bin/env python3
"""Device cost of cloud segmentation, one JSON line per measurement: fdm_cloud_segment_ground,
fdm_cloud_segment_plane and fdm_cloud_segment_planes on device-resident clouds — the 28.8 K-point VLP-16 scan, the
272 K-point RGB-D frame and the 2.1 M-point 128-beam scan of fastdem_amd.synth, in their sensor frames, the points
with a coordinate that is not finite dropped first (segment_ground refuses them).

ms = median over --repeat calls of the four device intervals fdm_segment_last_stats reports (fdm_cloud_debug_profile
switches the events on; what each interval holds: include/fdm_engine.h) and their sum; wall_ms = the whole synchronous
call, allocations, read-backs and those events included.  segment_plane is measured at --batches hypotheses per launch
(fdm_segment_debug_batch); its line carries the loop passes the run made and the launches they took.  restate_ms = the
wall time of the NumPy restatement (tests/seg_restate.py) on this host, for clouds of up to --restate-max points.

  python scripts/segment_bench.py [--repeat 7] [--out profiles/r12/segment/segment_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLANE = dict(distance_threshold=0.1, max_iterations=1000, probability=0.99)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--clouds", default="vlp16,rgbd,lidar128")
    ap.add_argument("--batches", default="32,64,128")
    ap.add_argument("--restate-max", type=int, default=300000)
    args = ap.parse_args()
    import torch
    import fastdem_amd as F
    import seg_restate as SR
    lib = F.capi.load()
    lib.fdm_cloud_debug_profile(1)
    lines = []

    def measure(fn, **tags):
        fn()  # warm-up: code objects, the allocator
        parts, wall, st = [], [], None
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = F.segment_last_stats()
            parts.append(st["ms"])
        med = np.median(np.asarray(parts), axis=0)
        line = dict(tags, stage_ms=[round(float(v), 4) for v in med],
                    ms=round(float(np.median(np.asarray(parts).sum(axis=1))), 4), wall_ms=round(float(np.median(wall)), 3),
                    n_batches=st["n_batches"], n_hypotheses=st["n_hypotheses"], batch=st["batch"])
        return out, line

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for name in args.clouds.split(","):
        s = F.synth.make(name, n_scans=1).scan(0)
        ok = np.isfinite(s["x"]) & np.isfinite(s["y"]) & np.isfinite(s["z"])
        host = tuple(np.ascontiguousarray(s[k][ok], dtype=np.float32) for k in ("x", "y", "z"))
        dev = tuple(torch.from_numpy(v).cuda() for v in host)
        n = int(host[0].size)
        restate = n <= args.restate_max

        (g, o), line = measure(lambda: F.segment_ground(*dev), call="segment_ground", cloud=name, n=n)
        line.update(n_ground=int(g.numel()), n_obstacles=int(o.numel()))
        if restate:
            t0 = time.perf_counter()
            rg, ro = SR.segment_ground(*host)
            line["restate_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            line["equal"] = bool(np.array_equal(g.cpu().numpy(), rg) and np.array_equal(o.cpu().numpy(), ro))
        emit(line)

        for batch in (int(b) for b in args.batches.split(",")):
            lib.fdm_segment_debug_batch(batch)
            r, line = measure(lambda: F.segment_plane(*dev, **PLANE), call="segment_plane", cloud=name, n=n)
            line.update(iterations=r.iterations, n_inliers=int(r.inliers.numel()), fitness=round(r.fitness, 6))
            if restate and batch == 128:
                t0 = time.perf_counter()
                rr = SR.segment_plane(*host, **PLANE)
                line["restate_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                line["equal"] = bool(rr["iterations"] == r.iterations and np.array_equal(r.inliers.cpu().numpy(), rr["inliers"]))
            emit(line)
        lib.fdm_segment_debug_batch(0)

        res, line = measure(lambda: F.segment_multiple_planes(*dev, max_planes=3, min_fitness=0.05, **PLANE),
                            call="segment_multiple_planes", cloud=name, n=n)
        line.update(planes=len(res), iterations=[r.iterations for r in res], n_inliers=[int(r.inliers.numel()) for r in res])
        emit(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
