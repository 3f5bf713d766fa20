#!/usr/bin/env python3
"""Device cost of Euclidean clustering, one JSON line per measurement: fdm_cloud_cluster on device-resident
clouds — the 28.8 K-point VLP-16 scan, the 272 K-point RGB-D frame and the 2.1 M-point 128-beam scan of
fastdem_amd.synth, in their sensor frames, the points with a coordinate that is not finite dropped first — each after
segment_ground, with its obstacle list as the subset, at tolerance 0.5 (the reference's lidar_perception chain).

stage_ms = median over --repeat calls of the six device intervals fdm_cluster_last_stats reports (fdm_cloud_debug_profile
switches the events on; what each interval holds: include/fdm_engine.h), ms their sum; wall_ms = the whole synchronous
call, allocations, read-backs and those events included.  restate_ms = the wall time of the NumPy / Python restatement
(tests/cluster_restate.py) on this host, for lists of up to --restate-max points: a sanity figure, not a claim.

--dense N1,N2,...: the work bound's measurement.  N points inside ONE voxel (a cube of 0.45 at tolerance 0.5: N (N - 1) / 2
candidate pairs, most of them neighbours); sizes are taken in order and the series stops after the first call whose merge
took more than --dense-stop-ms.

  python scripts/cluster_bench.py [--repeat 7] [--dense 32768,131072,262144] [--out profiles/r13/cluster/cluster_bench.jsonl]
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

CLUSTER = dict(tolerance=0.5, min_size=10, max_size=100000)
COUNTS = ("n_points", "n_components", "n_kept", "n_clustered", "candidate_pairs", "neighbour_pairs", "unions", "key_bits")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--clouds", default="vlp16,rgbd,lidar128")
    ap.add_argument("--dense", default="")
    ap.add_argument("--dense-stop-ms", type=float, default=400.0)
    ap.add_argument("--restate-max", type=int, default=40000)
    args = ap.parse_args()
    import torch
    import fastdem_amd as F
    import cluster_restate as CR
    lib = F.capi.load()
    lib.fdm_cloud_debug_profile(1)
    lines = []

    def measure(fn, repeat, **tags):
        fn()  # warm-up: code objects, the allocator
        parts, wall, st = [], [], None
        for _ in range(repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = F.cluster_last_stats()
            parts.append(st["ms"])
        med = np.median(np.asarray(parts), axis=0)
        line = dict(tags, stage_ms=[round(float(v), 4) for v in med],
                    ms=round(float(np.median(np.asarray(parts).sum(axis=1))), 4), wall_ms=round(float(np.median(wall)), 3),
                    **{k: st[k] for k in COUNTS})
        return out, line

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for name in [c for c in args.clouds.split(",") if c]:
        s = F.synth.make(name, n_scans=1).scan(0)
        ok = np.isfinite(s["x"]) & np.isfinite(s["y"]) & np.isfinite(s["z"])
        host = tuple(np.ascontiguousarray(s[k][ok], dtype=np.float32) for k in ("x", "y", "z"))
        dev = tuple(torch.from_numpy(v).cuda() for v in host)
        n = int(host[0].size)
        _, obstacles = F.segment_ground(*dev)
        r, line = measure(lambda: F.euclidean_cluster(*dev, indices=obstacles, **CLUSTER), args.repeat,
                          call="euclidean_cluster", cloud=name, n=n)
        sizes = r.cluster_sizes().cpu().numpy()
        line.update(largest=[int(v) for v in sizes[:3]])
        if int(obstacles.numel()) <= args.restate_max:
            idx = obstacles.cpu().numpy().astype(np.uint32)
            t0 = time.perf_counter()
            _, _, clusters = CR.euclidean_cluster(*host, indices=idx, **CLUSTER)
            line["restate_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            want_ind, want_off, _ = CR.canonical(clusters, idx, idx.size)
            line["equal"] = bool(np.array_equal(r.indices.cpu().numpy(), want_ind) and
                                 np.array_equal(r.offsets.cpu().numpy(), want_off))
        emit(line)

    rng = np.random.default_rng(1)
    for n in [int(v) for v in args.dense.split(",") if v]:
        pts = (np.round(rng.uniform(0.0, 0.45, (n, 3)) * 1024.0) / 1024.0).astype(np.float32)
        dev = tuple(torch.from_numpy(np.ascontiguousarray(pts[:, k])).cuda() for k in range(3))
        r, line = measure(lambda: F.euclidean_cluster(*dev, tolerance=0.5, min_size=1, max_size=n), 2,
                          call="dense_voxel", n=n)
        merge_ms = line["stage_ms"][3]
        line.update(pairs_per_s=round(line["candidate_pairs"] / max(merge_ms, 1e-6) * 1e3, 0))
        emit(line)
        if merge_ms > args.dense_stop_ms:
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
