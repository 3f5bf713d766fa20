"""buildDEM on the device (fastdem_amd/csrc/fdm_engine_dem.inl) and its histogram filter (fdm_dem.hpp) against the NumPy
restatement of fastdem/src/pcd_convert.cpp:194-323 (tests/dem_restate.py): the keep mask of removeFloatingPoints equal;
of the full pipeline every layer, the geometry and the stage counts bit for bit.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import functools

import numpy as np
import pytest

import dem_restate as DR
from helpers import assert_layers_bit_identical

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H, RES = 4.0, 3.0, 0.1        # 40 x 30 cells


def centre(r, c):
    return W / 2 - (r + 0.5) * RES, H / 2 - (c + 0.5) * RES


def filter_cloud():
    """Rows 0-19: noisy ground with a canopy 3 m up over a part of it.  Rows 22-39: hand-made cells."""
    rng = np.random.default_rng(31)
    n = 1500
    x = rng.uniform(0.0, W / 2, n)
    y = rng.uniform(-H / 2, H / 2, n)
    z = rng.normal(0.0, 0.03, n)
    xc, yc = rng.uniform(0.5, 1.5, 300), rng.uniform(-1.0, 1.0, 300)   # canopy
    pts = [np.stack([x, y, z], 1), np.stack([xc, yc, rng.normal(3.0, 0.05, 300)], 1)]

    def cell(r, c, zs):
        cx, cy = centre(r, c)
        m = len(zs)
        pts.append(np.stack([cx + rng.uniform(-0.04, 0.04, m), cy + rng.uniform(-0.04, 0.04, m), np.asarray(zs)], 1))

    for k in range(12):                                              # cells with one point
        cell(22 + k, 2, [rng.normal(1.0, 1.0)])
    cell(24, 6, [2.5] * 7)                                           # all-equal z: one bin
    cell(26, 6, [0.01, 0.02, 1.01, 1.02, 0.51, 3.5])                 # two equal peaks: the lowest wins, 3.5 goes
    cell(26, 10, [1.01, 1.02, 0.01, 0.02, 0.51, 3.5])                # ... in whichever order they come
    bin32, ht = F32(RES), F32(2.0)
    cutoff = F32(F32(F32(0.0) + F32(F32(0.5) * bin32)) + ht)         # z_min 0, bin 0
    cell(28, 6, [0.0, 0.0, 0.0, cutoff, np.nextafter(cutoff, F32(9))])   # exactly at the cutoff: kept; one ulp above: not
    cell(30, 6, list(rng.uniform(0.0, 0.05, 40)) + list(rng.uniform(5.0, 5.05, 39)))   # 40 below, 39 above
    cell(32, 6, [np.nan, 1.0, 1.0])                                  # a NaN z is skipped
    p = np.concatenate(pts)
    p = p[rng.permutation(len(p))]
    p = np.concatenate([p, [[9.0, 0.0, 1.0], [np.nan, 0.0, 1.0]]])   # outside the map, no cell
    return p[:, 0].astype(F32), p[:, 1].astype(F32), p[:, 2].astype(F32)


@functools.lru_cache(maxsize=None)
def restated_filter(height_threshold, bin_size):
    import fdm_ref_py as R
    x, y, z = filter_cloud()
    grid = R.RefEngine(float(F32(W)), float(F32(H)), float(F32(RES)))
    keep = DR.restate_floating(grid, x, y, z, height_threshold, F32(bin_size) if bin_size > 0 else F32(RES))
    keep.setflags(write=False)
    return (x, y, z), keep


@pytest.mark.parametrize("height_threshold,bin_size", [(2.0, 0.0), (2.0, 0.25), (0.5, 0.0), (0.5, 0.03)])
def test_floating_point_removal(gpu, R, height_threshold, bin_size):
    (x, y, z), keep = restated_filter(height_threshold, bin_size)
    assert 0 < keep.sum() < keep.size and not keep[-2:].any()
    if (height_threshold, bin_size) == (2.0, 0.0):
        canopy = (z > 2.8) & (z < 3.3) & (x > 0.5) & (x < 1.5)
        assert 0 < keep[canopy].mean() < 0.5      # the canopy 3 m up goes, except over cells without a ground point
    eng = gpu.Engine.create_map(W, H, RES)
    got = eng.remove_floating_points(x, y, z, height_threshold, bin_size)
    bad = np.flatnonzero(got != keep)
    assert bad.size == 0, f"{bad.size} points differ, e.g. {bad[:5]} z={z[bad[:5]]}"
    assert eng.layers() == ["elevation", "elevation_min", "elevation_max"] and np.isnan(eng.layer("elevation")).all()
    import torch
    d = [torch.from_numpy(v).cuda() for v in (x, y, z)]
    assert np.array_equal(eng.remove_floating_points(*d, height_threshold, bin_size).cpu().numpy().astype(bool), keep)
    eng.close()


def test_floating_point_removal_refuses_a_bin_count_beyond_int32(gpu, R):
    eng = gpu.Engine.create_map(W, H, RES)
    x, y = np.zeros(2, dtype=F32), np.zeros(2, dtype=F32)
    with pytest.raises(gpu.EngineError):
        eng.remove_floating_points(x, y, np.array([0.0, 3e9], dtype=F32), 2.0, 1.0)
    assert eng.remove_floating_points(x, y, np.array([0.0, 2e9], dtype=F32), 2.0, 1.0).tolist() == [True, False]
    eng.close()


# ---- the whole pipeline ----
def dem_cloud():
    """A 6 x 4 m slope with noise, a canopy over a part of it, a hole inpainting closes, a few far outliers."""
    rng = np.random.default_rng(41)
    n = 1400
    x, y = rng.uniform(-3.0, 3.0, n), rng.uniform(-2.0, 2.0, n)
    hole = (np.abs(x - 1.0) < 0.3) & (np.abs(y) < 0.3)
    x, y = x[~hole], y[~hole]
    z = 0.1 * x + rng.normal(0.0, 0.02, x.size)
    xc, yc = rng.uniform(-2.5, -1.0, 250), rng.uniform(-1.5, 1.5, 250)
    xo, yo, zo = rng.uniform(-3, 3, 6), rng.uniform(-2, 2, 6), rng.uniform(8.0, 15.0, 6)
    p = np.concatenate([np.stack([x, y, z], 1), np.stack([xc, yc, rng.normal(3.0, 0.05, 250)], 1),
                        np.stack([xo, yo, zo], 1)])
    p = p[rng.permutation(len(p))].astype(F32)
    m = len(p)
    return {"x": p[:, 0].copy(), "y": p[:, 1].copy(), "z": p[:, 2].copy(),
            "intensity": rng.uniform(0, 1, m).astype(F32), "rgb": rng.integers(0, 1 << 24, m).astype(np.uint32)}


PIPELINES = [("max", True, 0, False), ("max", False, 3, True), ("min", True, 3, False), ("min", False, 0, True),
             ("mean", True, 3, True), ("mean", False, 0, False), ("minmax", True, 0, True), ("minmax", False, 3, False)]
CONFIG = dict(resolution=0.2, sor_k=8, sor_std_mul=1.5, height_threshold=1.0, bin_size=0.0)


@functools.lru_cache(maxsize=None)
def restated_dem(method, channels, inpaint):
    import fdm_ref_py as R
    c = dem_cloud()
    dem = DR.restate_build_dem(R, c["x"], c["y"], c["z"], c["intensity"] if channels else None,
                               c["rgb"] if channels else None, method=method, inpaint_iterations=inpaint, **CONFIG)
    assert dem is not None and dem.n_after_height < dem.n_after_sor < c["x"].size
    for a in dem.store.values():
        a.setflags(write=False)
    return c, dem


@pytest.mark.parametrize("method,channels,inpaint,on_device", PIPELINES)
def test_build_dem(gpu, R, method, channels, inpaint, on_device):
    c, dem = restated_dem(method, channels, inpaint)
    names = ("x", "y", "z") + (("intensity", "rgb") if channels else ())
    arrays = {k: c[k] for k in names}
    if on_device:
        import torch
        arrays = {k: torch.from_numpy(v.view(np.int32) if k == "rgb" else v).cuda() for k, v in arrays.items()}
    cfg = gpu.DEMConfig(method=method, inpaint_iterations=inpaint, **CONFIG)
    eng, st = gpu.build_dem(arrays["x"], arrays["y"], arrays["z"], arrays.get("intensity"), arrays.get("rgb"), config=cfg,
                            return_stats=True)
    assert eng is not None and st["status"] == 0
    assert (st["n_input"], st["n_after_sor"], st["n_after_height"]) == (c["x"].size, dem.n_after_sor, dem.n_after_height)
    assert F32(st["sor_threshold"]).view(np.uint32) == F32(dem.threshold).view(np.uint32)
    assert st["n_points_used"] == int(dem.layer("n_points").sum())
    assert st["n_cells_written"] == int((dem.layer("n_points") > 0).sum())
    g = eng.geometry()
    assert (g.length_x, g.length_y, g.resolution, g.position_x, g.position_y, g.rows, g.cols) == dem.geometry
    assert (g.start_row, g.start_col) == (0, 0)
    assert eng.layers() == dem.layers()
    assert_layers_bit_identical(eng, dem)
    if inpaint:
        assert np.isnan(dem.layer("elevation_min")).sum() > np.isnan(dem.layer("elevation")).sum()   # holes were closed
    eng.close()


def test_build_dem_without_a_map(gpu):
    e = np.zeros(0, dtype=F32)
    eng, st = gpu.build_dem(e, e, e, return_stats=True)
    assert eng is None and st["status"] == gpu.capi.FDM_SKIP_EMPTY_CLOUD
    one = np.ones(1, dtype=F32)
    eng, st = gpu.build_dem(one, one, one, return_stats=True)
    assert eng is None and st["status"] == gpu.capi.FDM_SKIP_ALL_FILTERED
    c = dem_cloud()
    eng, st = gpu.build_dem(c["x"], c["y"], c["z"], config=gpu.DEMConfig(sor_k=0), return_stats=True)
    assert eng is None and st["status"] == gpu.capi.FDM_SKIP_ALL_FILTERED
    assert gpu.build_dem(e, e, e) is None


def test_build_dem_refusals(gpu):
    c = dem_cloud()
    with pytest.raises(gpu.EngineError):                             # more than 64 neighbours
        gpu.build_dem(c["x"], c["y"], c["z"], config=gpu.DEMConfig(sor_k=65))
    z = c["z"].copy()
    z[5] = np.nan
    with pytest.raises(gpu.EngineError):
        gpu.build_dem(c["x"], c["y"], z)
