#!/usr/bin/env python3
"""Device cost of the cloud filters, one JSON line per measurement, on device-resident clouds: the 272 K-point
RGB-D frame and the 2.1 M-point 128-beam scan of fastdem_amd.synth, in their sensor frames, the points with a coordinate
that is not finite dropped first (by remove_invalid, which is timed too).

radius_outlier_removal at radii 0.1, 0.3 and 1.0 with min_neighbors 5, in mask mode and in count mode: stage_ms = median
over --repeat calls of the five device intervals fdm_ror_last_stats reports (fdm_cloud_debug_profile switches the events
on; what each interval holds: include/fdm_engine.h), ms their sum; wall_ms = the whole synchronous call, allocations,
read-backs and those events included.  tests_per_s = tests_done over the count kernel's interval: in count mode the
candidate rate the work bound (filter::kMaxTests, fdm_filter_host.hpp) is held against.  A call the work bound refuses is
reported as refused, with its candidate tests.  equal = mask mode's keep is count mode's counts >= min_neighbors.

One crop of each kind: wall_ms of the synchronous call (one elementwise kernel, its allocation and the read-back of the
count).  For orientation euclidean_cluster at tolerance 0.5 over the whole frame — it shares the front half (voxels, sort,
gather) with the radius outlier removal.

--dense N1,N2,...: the work bound's measurement, N points inside ONE voxel in count mode (see the loop's comment).

  python scripts/filters_bench.py [--repeat 7] [--clouds rgbd,lidar128] [--dense 65536,131072,262144]
                                  [--out profiles/r20/filters/filters_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADII = (0.1, 0.3, 1.0)
MIN_NEIGHBORS = 5
COUNTS = ("n_points", "candidate_tests", "tests_done", "n_kept", "range", "key_bits")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--clouds", default="rgbd,lidar128")
    ap.add_argument("--dense", default="")
    ap.add_argument("--dense-stop-ms", type=float, default=400.0)
    ap.add_argument("--slow-ms",type=float, default=300.0, help="a call slower than this is repeated twice only")
    args = ap.parse_args()
    import torch
    import fastdem_amd as F
    lib = F.capi.load()
    lib.fdm_cloud_debug_profile(1)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    def timed(fn, repeat, stats=None):
        """(the last result, median wall ms, the median of stats()["ms"] over the calls and the last stats)"""
        fn()  # warm-up: code objects, the allocator
        wall, parts, st, out = [], [], None, None
        for k in range(repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            if stats:
                st = stats()
                parts.append(st["ms"])
            if wall[-1] > args.slow_ms and k >= 1:
                break
        med = np.median(np.asarray(parts), axis=0) if parts else None
        return out, float(np.median(wall)), med, st

    for name in [c for c in args.clouds.split(",") if c]:
        s = F.synth.make(name, n_scans=1).scan(0)
        raw = tuple(torch.from_numpy(np.ascontiguousarray(s[k], dtype=np.float32)).cuda() for k in ("x", "y", "z"))
        ok, wall, _, _ = timed(lambda: F.remove_invalid(*raw), args.repeat)
        emit(dict(call="remove_invalid", cloud=name, n=int(raw[0].numel()), kept=int(ok.sum()), wall_ms=round(wall, 3)))
        dev = tuple(v[ok.bool()].contiguous() for v in raw)
        n = int(dev[0].numel())
        torch.cuda.synchronize()

        for radius in RADII:
            results = {}
            for mode in ("mask", "count"):
                call = lambda: F.radius_outlier_removal(*dev, radius, MIN_NEIGHBORS, return_counts=mode == "count")  # noqa: E731
                tags = dict(call="radius_outlier_removal", mode=mode, cloud=name, n=n, radius=radius, min_neighbors=MIN_NEIGHBORS)
                try:
                    out, wall, med, st = timed(call, args.repeat, F.ror_last_stats)
                except F.EngineError as e:
                    st = F.ror_last_stats()
                    emit(dict(tags, refused=str(e)[:120], candidate_tests=st["candidate_tests"]))
                    continue
                results[mode] = out
                line = dict(tags, stage_ms=[round(float(v), 4) for v in med], ms=round(float(med.sum()), 4),
                            wall_ms=round(wall, 3), **{k: st[k] for k in COUNTS})
                line["tests_per_s"] = round(st["tests_done"] / max(float(med[3]), 1e-6) * 1e3, 0)
                emit(line)
            if len(results) == 2:
                keep_c, counts = results["count"]
                emit(dict(call="radius_outlier_removal", cloud=name, radius=radius,
                          equal=bool(torch.equal(results["mask"], keep_c) and
                                     torch.equal(keep_c.bool(), counts >= MIN_NEIGHBORS))))

        crops = (("crop_box", ((-5.0, -5.0, -1.0), (5.0, 5.0, 2.0))), ("crop_range", (1.0, 20.0)), ("crop_x", (0.0, 10.0)),
                 ("crop_y", (-3.0, 3.0)), ("crop_z", (-1.0, 1.0)), ("crop_angle", (-0.7853982, 0.7853982)))
        for fn, a in crops:
            keep, wall, _, _ = timed(lambda: getattr(F, fn)(*dev, *a), args.repeat)
            emit(dict(call=fn, cloud=name, n=n, kept=int(keep.sum()), wall_ms=round(wall, 3)))

        try:
            r, wall, med, st = timed(lambda: F.euclidean_cluster(*dev, tolerance=0.5, min_size=10, max_size=n),
                                     args.repeat, F.cluster_last_stats)
            emit(dict(call="euclidean_cluster", cloud=name, n=n, tolerance=0.5, stage_ms=[round(float(v), 4) for v in med],
                      ms=round(float(med.sum()), 4), wall_ms=round(wall, 3), candidate_pairs=st["candidate_pairs"],
                      clusters=r.num_clusters))
        except F.EngineError as e:
            emit(dict(call="euclidean_cluster", cloud=name, n=n, tolerance=0.5, refused=str(e)[:120]))
    # the work bound's measurement: N points inside ONE voxel (a cube of 0.45 at radius 0.5: N (N - 1) candidate tests,
    # most of them neighbours), count mode; the series stops after the first call whose count kernel took --dense-stop-ms
    rng = np.random.default_rng(1)
    for n in [int(v) for v in args.dense.split(",") if v]:
        pts = (np.round(rng.uniform(0.0, 0.45, (n, 3)) * 1024.0) / 1024.0).astype(np.float32)
        dev = tuple(torch.from_numpy(np.ascontiguousarray(pts[:, k])).cuda() for k in range(3))
        _, wall, med, st = timed(lambda: F.radius_outlier_removal(*dev, 0.5, MIN_NEIGHBORS, return_counts=True), 2,
                                 F.ror_last_stats)
        emit(dict(call="dense_voxel", mode="count", n=n, stage_ms=[round(float(v), 4) for v in med], wall_ms=round(wall, 3),
                  candidate_tests=st["candidate_tests"], tests_per_s=round(st["tests_done"] / max(float(med[3]), 1e-6) * 1e3, 0)))
        if med[3] > args.dense_stop_ms:
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
