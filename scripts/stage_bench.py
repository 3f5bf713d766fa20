#!/usr/bin/env python3
"""Device time of the stages either side of the hot path (SURVEY.md §8 f3 egress, f4 ingest), with the
algorithmic bytes each moves and the CPU oracle beside it.   python scripts/stage_bench.py [c2|c4]
One JSON line per stage.  Timing: HIP events on the engine's... the entry points are synchronous
(they return counts), so wall time of the call with inputs resident in HBM is reported, plus the
kernel-only time from rocprofv3 when run under scripts/prof_stages.sh."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from fastdem_amd import synth  # noqa: E402
from cloud2 import make_blob  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="c4")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--cpu-iters", type=int, default=3)
ap.add_argument("--only", default=None, choices=["raster", "dem"],
                help="'raster': the fromPointCloud row, and nothing else; 'dem': the buildDEM row, and nothing else")
a = ap.parse_args()
wl = synth.make(a.workload)
res = bench.Resident(wl, 0)
for k in range(12):
    res.step(k)
res.eng.sync()
eng = res.eng
HBM = 8.0e12


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


# ---- fromPointCloud: the workload's first scan as a static world-frame cloud, rasterized from device arrays onto a
# map-only engine of the workload's size; beside it fdm_engine_integrate_device of the same cloud on the same map size ----
def raster_row():
    from fastdem_amd import Engine
    s = wl.scan(0)
    T = (wl.pose(0) @ wl.T_base_sensor).astype(np.float64)
    p = np.stack([s["x"], s["y"], s["z"], np.ones_like(s["x"])]).astype(np.float64)
    w = (T @ p).astype(np.float32)
    d = [torch.from_numpy(np.ascontiguousarray(w[k])).cuda() for k in range(3)]
    di = None if s["intensity"] is None else torch.from_numpy(s["intensity"]).cuda()
    m = Engine.create_map(wl.width, wl.height, wl.resolution)
    m.enable_profile()
    rc, st = m.from_point_cloud(d[0], d[1], d[2], intensity=di, method="mean")
    assert rc == 0, rc
    t_call = timed(lambda: m.from_point_cloud(d[0], d[1], d[2], intensity=di, method="mean"), a.iters)
    ids_ms, group_ms, walk_ms = m.last_raster_ms()
    counts = m.layer("n_points")
    res.eng.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        res.step(0)
    res.eng.sync()
    t_int = (time.perf_counter() - t0) / a.iters
    print(json.dumps({"stage": "from_point_cloud (device arrays, mean)", "workload": a.workload, "points": int(s["x"].size),
                      "cells": m.rows * m.cols, "points_used": st["n_points_used"], "cells_written": st["n_cells_written"],
                      "max_points_per_cell": int(counts.max()), "call_ms": round(t_call * 1e3, 4),
                      "ids_ms": round(ids_ms, 4), "grouping_ms": round(group_ms, 4), "walk_ms": round(walk_ms, 4),
                      "integrate_device_ms": round(t_int * 1e3, 4), "ratio": round(t_call / t_int, 2)}))


# ---- buildDEM: the same world-frame cloud through the whole offline pipeline with the default DEMConfig, from device
# arrays; per stage the device ms fdm_dem_stats reports, the call's wall time beside their sum ----
def dem_row():
    import fastdem_amd
    s = wl.scan(0)
    T = (wl.pose(0) @ wl.T_base_sensor).astype(np.float64)
    p = np.stack([s["x"], s["y"], s["z"], np.ones_like(s["x"])]).astype(np.float64)
    w = (T @ p).astype(np.float32)
    d = [torch.from_numpy(np.ascontiguousarray(w[k])).cuda() for k in range(3)]
    di = None if s["intensity"] is None else torch.from_numpy(s["intensity"]).cuda()
    cfg = fastdem_amd.DEMConfig()
    best = None
    for _ in range(3):                     # the first call pays the allocations' first touch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, st = fastdem_amd.build_dem(d[0], d[1], d[2], intensity=di, config=cfg, return_stats=True)
        wall = (time.perf_counter() - t0) * 1e3
        sor = fastdem_amd.sor_last_stats()
        if best is None or wall < best[0]:
            best = (wall, st, sor, (m.rows, m.cols) if m is not None else None)
        if m is not None:
            m.close()
    wall, st, sor, shape = best
    names = ("knn_grid_ms", "knn_search_ms", "knn_fallback_ms", "sor_statistics_ms", "height_filter_ms", "raster_ms",
             "inpaint_ms")
    row = {"stage": "build_dem (device arrays, default DEMConfig)", "workload": a.workload, "points": int(s["x"].size),
           "map": shape, "n_after_sor": st["n_after_sor"], "n_after_height": st["n_after_height"],
           "fallback_queries": st["n_sor_fallback"], "fallback_share": round(st["n_sor_fallback"] / max(1, s["x"].size), 6),
           "knn_grid": (sor["grid_x"], sor["grid_y"]), "knn_column_m": round(sor["voxel"], 5),
           "call_ms": round(wall, 3), "stages_ms": round(sum(st["stage_ms"]), 3)}
    row.update({k: round(v, 4) for k, v in zip(names, st["stage_ms"])})
    print(json.dumps(row))


if a.only == "dem":
    dem_row()
    sys.exit(0)
if a.only == "raster":   # (a second 1200 x 1200 engine and 20 synchronous calls: only when asked for)
    raster_row()
    sys.exit(0)

# ---- egress: toPointCloud2 compaction + packing, records stay in HBM ----
d_ptr, n_pts, step = eng.pack_cloud_device()
t = timed(lambda: eng.pack_cloud_device(), a.iters)
cells = eng.rows * eng.cols
nf = step // 4
alg = cells * 4 * 2 + n_pts * ((nf - 2) * 4 + step)  # elevation read by count+fill, layers read, records written
import fdm_ref_py as R  # noqa: E402  (CPU baseline only)
ref = R.RefEngine(wl.width, wl.height, wl.resolution, wl.apply_to(R.default_config()))
for name in eng.layers():
    ref.set_layer(name, eng.layer(name))
g = eng.geometry()
ref.set_position(g.position_x, g.position_y)
ref.set_start_index(g.start_row, g.start_col)
t0 = time.perf_counter()
for _ in range(a.cpu_iters):
    f_ref, s_ref, d_ref = ref.pack_cloud()
t_cpu = (time.perf_counter() - t0) / a.cpu_iters
assert d_ref.shape[0] == n_pts and s_ref == step
print(json.dumps({"stage": "egress_pack_cloud", "workload": a.workload, "cells": cells, "points_out": n_pts,
                  "point_step": step, "gpu_ms": round(t * 1e3, 4), "algorithmic_MB": round(alg / 1e6, 2),
                  "GBps": round(alg / t / 1e9, 1), "hbm_frac": round(alg / t / HBM, 4),
                  "cpu_oracle_ms": round(t_cpu * 1e3, 2), "speedup": round(t_cpu / t, 1)}))

# ---- render: one layer -> RGBA8 image (savePng's pixels; radix select for the 1 % / 99 % range + colour map) beside the
# download of the same layer, the only route to those pixels without the stage ----
t_dev = timed(lambda: eng.render_layer_device("elevation", want_range=False), a.iters)   # image stays in HBM
t_host = timed(lambda: eng.render_layer("elevation"), a.iters)                            # + range + one RGBA copy out
t_down = timed(lambda: eng.layer("elevation"), a.iters)
alg = cells * 4 * 5 + cells * 4   # four digit passes + the colour pass read the layer, the image is written once
print(json.dumps({"stage": "render (percentile_1_99, viridis)", "workload": a.workload, "cells": cells,
                  "gpu_ms": round(t_dev * 1e3, 4), "to_host_ms": round(t_host * 1e3, 4),
                  "layer_download_ms": round(t_down * 1e3, 4), "algorithmic_MB": round(alg / 1e6, 2),
                  "GBps": round(alg / t_dev / 1e9, 1), "hbm_frac": round(alg / t_dev / HBM, 4)}))

# ---- ingest: PointCloud2 blob (32-byte records, x y z _ intensity ring time) already in HBM ----
s = wl.scans[0]
blob, lay = make_blob(s["x"], s["y"], s["z"], intensity=s["intensity"] if s["intensity"] is not None else np.zeros_like(s["x"]),
                      offsets=dict(x=0, y=4, z=8, intensity=16), point_step=32)
n = s["x"].size
d_blob = torch.from_numpy(np.ascontiguousarray(blob)).cuda()
layout = eng.cloud2_layout(lay.point_step, lay.off_x, lay.off_y, lay.off_z, lay.off_intensity, lay.intensity_type, lay.off_rgb)
import ctypes as C  # noqa: E402
nv = C.c_uint64(0)


def ingest():
    rc = eng._lib.fdm_engine_ingest_cloud2(eng._h, C.c_void_p(d_blob.data_ptr()), 1, n, C.byref(layout), C.byref(nv))
    assert rc == 0


t = timed(ingest, a.iters)
alg = n * 32 + n * 12 + nv.value * 16  # records read (count pass reads xyz only), SoA written
t0 = time.perf_counter()
for _ in range(a.cpu_iters):
    c_ref = R.from_cloud2(blob, n, lay)
t_cpu = (time.perf_counter() - t0) / a.cpu_iters
assert c_ref["x"].size == nv.value
print(json.dumps({"stage": "ingest_cloud2", "workload": a.workload, "points": n, "kept": nv.value, "point_step": 32,
                  "gpu_ms": round(t * 1e3, 4), "algorithmic_MB": round(alg / 1e6, 2), "GBps": round(alg / t / 1e9, 1),
                  "hbm_frac": round(alg / t / HBM, 4), "cpu_oracle_ms": round(t_cpu * 1e3, 2),
                  "speedup": round(t_cpu / t, 1)}))

# ---- message -> map in one call (from_impl + integrate, fdm_engine_integrate_cloud2): one decode kernel +
# the scan, no host round trip in between; blob in HBM / pinned message decoded over PCIe / pageable message
import fastdem_amd  # noqa: E402
eng2 = bench.Resident(wl, 0).eng
tbs = bench.colmajor16(wl.T_base_sensor)
twb = bench.colmajor16(wl.pose(0))
st2 = fastdem_amd.capi.FdmScanStats()
pin_msg = fastdem_amd.host_array(np.frombuffer(blob, dtype=np.uint8), dtype=np.uint8)
page_msg = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8)).copy()


def msg_call(ptr, on_dev):
    def f():
        rc = eng2._lib.fdm_engine_integrate_cloud2(eng2._h, C.c_void_p(ptr), on_dev, n, C.byref(layout), tbs, twb, C.byref(st2))
        assert rc == 0
    return f


t_hbm = timed(msg_call(d_blob.data_ptr(), 1), a.iters)
t_pin = timed(msg_call(pin_msg.array.ctypes.data, 0), a.iters)
t_page = timed(msg_call(page_msg.ctypes.data, 0), a.iters)
t0 = time.perf_counter()
for _ in range(a.cpu_iters):
    ref.integrate_cloud2(blob, n, lay, wl.T_base_sensor, wl.pose(0))
t_cpu = (time.perf_counter() - t0) / a.cpu_iters
print(json.dumps({"stage": "integrate_cloud2 (message -> map, synchronous)", "workload": a.workload, "points": n,
                  "point_step": 32, "gpu_ms_blob_in_hbm": round(t_hbm * 1e3, 4),
                  "gpu_ms_pinned_message": round(t_pin * 1e3, 4), "gpu_ms_pageable_message": round(t_page * 1e3, 4),
                  "cpu_oracle_ms": round(t_cpu * 1e3, 2), "speedup_pinned": round(t_cpu / t_pin, 1)}))

# ---- stencil post-processing on the mapped scene ----
for name, fn_gpu, fn_cpu, alg_bytes in (
        ("post_inpainting(3 passes)", lambda: eng.apply_inpainting(3, 2), lambda: ref.apply_inpainting(3, 2), cells * 4 * 2 * 4),
        ("post_median_3x3", lambda: eng.apply_spatial_smoothing("elevation_inpainted", 3, 5),
         lambda: ref.apply_spatial_smoothing("elevation_inpainted", 3, 5), cells * 4 * 3),
        ("post_uncertainty_fusion(r=0.15)", lambda: eng.apply_uncertainty_fusion(True, 0.15, 0.05, 0.01, 0.99, 3),
         lambda: ref.apply_uncertainty_fusion(True, 0.15, 0.05, 0.01, 0.99, 3), cells * 4 * 6),
        ("post_feature_extraction(r=0.3)", lambda: eng.apply_feature_extraction(0.3, 4, 0.05, 0.95),
         lambda: ref.apply_feature_extraction(0.3, 4, 0.05, 0.95), cells * 4 * 8)):
    t = timed(fn_gpu, max(3, a.iters // 4))
    t0 = time.perf_counter()
    fn_cpu()
    t_cpu = time.perf_counter() - t0
    print(json.dumps({"stage": name, "workload": a.workload, "cells": cells, "gpu_ms": round(t * 1e3, 4),
                      "algorithmic_MB": round(alg_bytes / 1e6, 2), "GBps": round(alg_bytes / t / 1e9, 1),
                      "cpu_oracle_ms": round(t_cpu * 1e3, 2), "speedup": round(t_cpu / t, 1)}))

# ---- the big neighbourhoods (k_median_sel / k_fusion_wave / k_features_sel; beyond the LDS: the pooled k_*_big), no CPU
# beside them; they exist so that no call the reference accepts is refused ----
res_cells = eng.rows * eng.cols
for name, fn_gpu, entries in (
        ("post_median_17x17 (k_median_sel)", lambda: eng.apply_spatial_smoothing("elevation_inpainted", 17, 5), 17 * 17),
        ("post_uncertainty_fusion(r=10 cells: 317 entries, k_fusion_wave)",
         lambda: eng.apply_uncertainty_fusion(True, 10.0 * wl.resolution + 1e-4, 0.05, 0.01, 0.99, 3), 317),
        ("post_feature_extraction(r=10 cells: 317 entries, k_features_sel)",
         lambda: eng.apply_feature_extraction(10.0 * wl.resolution + 1e-4, 4, 0.05, 0.95), 317)):
    t = timed(fn_gpu, 2)
    print(json.dumps({"stage": name, "workload": a.workload, "cells": res_cells, "entries_per_cell": entries,
                      "gpu_ms": round(t * 1e3, 3), "ns_per_cell": round(t * 1e9 / res_cells, 1)}))
