#!/usr/bin/env python3
"""Device cost of cloud registration, one JSON line per cloud and method: fdm_cloud_register (ICP,
point-to-plane ICP, GICP) and fdm_cloud_register_vgicp on device-resident clouds of the three sizes of BASELINE.json — the VLP-16 scan, the RGB-D
frame and the 128-beam scan of fastdem_amd.synth in the world frame — prepared on the device as a user would: voxelGrid
at --voxel metres, then normals and covariances at k = 20.  The target is that cloud; the source is the same cloud moved
by a known small transform (0.15 m, 0.02 rad) and rounded to float, registered from the identity.

Every method is run twice: on the source as voxelGrid leaves it (in voxel-key order, spatially coherent) and on the
same source shuffled (source_order), which is what a sort of the source by its target-grid key would undo.  Each call is
also repeated with max_iterations = 1: wall_per_iteration_ms = (wall_ms - wall_one_iteration_ms) / (linearizations - 1)
and wall_setup_ms = wall_one_iteration_ms - wall_per_iteration_ms separate the one-off work (allocations, staging, the
grid, the regularisation) from what an iteration costs end to end; first_iter_ms is the device time of that first
iteration, where the clouds are farthest apart.
Per line, medians over --repeat calls after one warm-up: grid_ms (the target's search grid, once per call),
regularize_ms (both clouds' GICP covariances, once per call), iter_ms (device time of one linearization — transform,
search, factor and the two sum kernels — the linearizations' total divided by their number), iterations, wall_ms (the
whole synchronous call: allocations, events, the host's 29-double read-back and 6 x 6 algebra per iteration included).
fdm_cloud_debug_profile switches the events on.  Not separated: search against factor inside the linearize kernel (one
kernel; the ICP line, whose factor is a dozen operations, is the closest to the search alone).

The vgicp lines register the same sources against a voxel distribution map of the target (--vgicp-voxel metres, built
ONCE per cloud and reused by every repeat, as scan-to-map registration does): map_ms is the map's build on the device
(keys + sort, reduce + regularise, hash: map_stage_ms), map_wall_ms the whole synchronous create call, grid_ms is 0,
regularize_ms the source's covariances alone; the other fields as for the other methods.

  python scripts/register_bench.py [--repeat 7] [--voxel 0.2] [--out profiles/register/register_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from normals_bench import world_cloud  # noqa: E402


def small_motion():
    """4 x 4: 0.15 m and 0.02 rad."""
    w = np.array([0.004, -0.008, 0.018])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = (0.1, -0.1, 0.05)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--max-dist", type=float, default=1.0)
    ap.add_argument("--vgicp-voxel", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--clouds", default="vlp16,rgbd,lidar128")
    args = ap.parse_args()
    import torch
    import fastdem_amd as F
    F.capi.load().fdm_cloud_debug_profile(1)
    gt = small_motion()
    inv = np.linalg.inv(gt)
    Ri = torch.from_numpy(inv[:3, :3]).cuda()
    ti = torch.from_numpy(inv[:3, 3]).cuda()
    lines = []
    for name in args.clouds.split(","):
        raw = [torch.from_numpy(v).cuda() for v in world_cloud(F, name)]
        down = F.voxel_grid(*raw, args.voxel)
        tgt = [down[c].contiguous() for c in ("x", "y", "z")]
        P = torch.stack(tgt, dim=1).double()
        S = (P @ Ri.T + ti).float()
        src = [S[:, a].contiguous() for a in range(3)]
        t_normals, t_cov = F.estimate_normals(*tgt, 20, covariances=True)
        _, s_cov = F.estimate_normals(*src, 20, covariances=True)
        perm = torch.randperm(src[0].numel(), device=src[0].device, generator=torch.Generator(device=src[0].device).manual_seed(1))
        shuf = [v[perm].contiguous() for v in src]
        shuf_cov = s_cov[perm].contiguous()
        md = args.max_dist
        calls = {("icp", "voxel"): lambda **kw: F.align_icp(*src, *tgt, max_correspondence_dist=md, **kw),
                 ("plane", "voxel"): lambda **kw: F.align_plane_icp(*src, *tgt, t_normals, max_correspondence_dist=md, **kw),
                 ("gicp", "voxel"): lambda **kw: F.align_gicp(*src, *tgt, s_cov, t_cov, max_correspondence_dist=md, **kw),
                 ("icp", "shuffled"): lambda **kw: F.align_icp(*shuf, *tgt, max_correspondence_dist=md, **kw),
                 ("plane", "shuffled"): lambda **kw: F.align_plane_icp(*shuf, *tgt, t_normals, max_correspondence_dist=md, **kw),
                 ("gicp", "shuffled"): lambda **kw: F.align_gicp(*shuf, *tgt, shuf_cov, t_cov, max_correspondence_dist=md, **kw)}
        # voxelized GICP: the map built once (timed over --repeat builds), then reused by every call
        F.VoxelMap(*tgt, resolution=args.vgicp_voxel).close()          # warm-up
        map_wall, map_ms = [], []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            probe = F.VoxelMap(*tgt, resolution=args.vgicp_voxel)
            map_wall.append((time.perf_counter() - t0) * 1e3)
            map_ms.append(probe.info()["ms"])
            probe.close()
        vmap = F.VoxelMap(*tgt, resolution=args.vgicp_voxel)
        info = vmap.info()
        calls[("vgicp", "voxel")] = lambda **kw: F.align_vgicp(*src, s_cov, voxel_map=vmap, **kw)
        calls[("vgicp", "shuffled")] = lambda **kw: F.align_vgicp(*shuf, shuf_cov, voxel_map=vmap, **kw)
        for (method, order), call in calls.items():
            call()                                                   # warm-up: code objects, the allocator
            ms, wall, wall1, first = [], [], [], []
            for _ in range(args.repeat):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                st = F.register_last_stats()
                ms.append((st["ms"][0], st["ms"][1], st["ms"][2] / max(1, st["linearizations"])))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(max_iterations=1)                               # the same call cut after its first iteration
                wall1.append((time.perf_counter() - t0) * 1e3)
                first.append(F.register_last_stats()["ms"][2])
            med = np.median(np.asarray(ms), axis=0)
            err = float(np.linalg.norm(res.transform @ inv - np.eye(4)))
            n_lin = max(2, st["linearizations"])
            wall_iter = (float(np.median(wall)) - float(np.median(wall1))) / (n_lin - 1)
            line = {"cloud": name, "method": method, "source_order": order, "n_raw": int(raw[0].numel()), "n": int(tgt[0].numel()),
                    "voxel_size": args.voxel, "max_dist": args.max_dist, "grid": [st["grid_x"], st["grid_y"]],
                    "column": round(st["voxel"], 5), "ring_limit": st["ring_limit"], "iterations": res.iterations,
                    "converged": res.converged, "fitness": round(res.fitness, 4), "error_to_truth": float(f"{err:.3e}"),
                    "grid_ms": round(float(med[0]), 4), "regularize_ms": round(float(med[1]), 4),
                    "iter_ms": round(float(med[2]), 4), "first_iter_ms": round(float(np.median(first)), 4),
                    "wall_ms": round(float(np.median(wall)), 3), "wall_one_iteration_ms": round(float(np.median(wall1)), 3),
                    "wall_per_iteration_ms": round(wall_iter, 4),
                    "wall_setup_ms": round(float(np.median(wall1)) - wall_iter, 3)}
            if method == "vgicp":
                stage = np.median(np.asarray(map_ms), axis=0)
                line.update({"map_voxel": args.vgicp_voxel, "map_voxels": int(info["num_voxels"]),
                             "map_sparse": int(info["n_sparse"]), "table_slots": int(info["table_slots"]),
                             "max_probe": int(info["max_probe"]), "map_ms": round(float(stage.sum()), 4),
                             "map_stage_ms": [round(float(v), 4) for v in stage],
                             "map_wall_ms": round(float(np.median(map_wall)), 3)})
            lines.append(line)
            print(json.dumps(line), flush=True)
        vmap.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
