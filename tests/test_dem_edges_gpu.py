"""Floating-point removal (fdm_dem.hpp, height_filter_device) and buildDEM (fdm_engine_dem.inl) at the limits of their two
radix sorts, of k_hf_peak's walk and of the order-keeping compaction, against the restatement of
fastdem/src/pcd_convert.cpp:194-323 (tests/dem_restate.py, tests/raster_restate.py): the keep mask equal, of the pipeline
every layer, the geometry and the stage counts bit for bit.  The clouds are tests/dem_cases.py's; which path each one
reaches is proved on the CPU in tests/test_dem_restate.py and not asserted again here.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

import dem_cases as DC
import test_build_dem_gpu as TB
from helpers import assert_layers_bit_identical, same_geometry

pytestmark = pytest.mark.gpu
F32 = np.float32


def engine_of(gpu, c):
    eng = gpu.Engine.create_map(*c.map)
    if c.move:
        eng.move(*c.move)
    return eng


def snapshot(eng, c):
    """A fresh map has its three basic layers, all NaN (a move is served as an empty scan, which brings the estimator's
    layers with it: of a moved map every layer is kept, to be compared bit for bit)."""
    if not c.move:
        assert eng.layers() == ["elevation", "elevation_min", "elevation_max"]
        return None
    return {k: eng.layer(k).copy() for k in eng.layers()}


def assert_untouched(eng, c, before):
    if before is None:
        assert eng.layers() == ["elevation", "elevation_min", "elevation_max"]
        assert all(np.isnan(eng.layer(k)).all() for k in eng.layers())
        return
    assert eng.layers() == list(before)
    for k, v in before.items():
        assert np.array_equal(eng.layer(k).view(np.uint32), v.view(np.uint32)), k


def assert_mask(got, keep, z):
    bad = np.flatnonzero(np.asarray(got, dtype=bool) != keep)
    assert bad.size == 0, f"{bad.size} of {keep.size} points differ, e.g. {bad[:5]} z={z[bad[:5]]} kept={keep[bad[:5]]}"
    assert np.array_equal(got, keep)


@pytest.mark.parametrize("name", DC.FILTER_CASES)
def test_floating_point_removal_at_the_limits(gpu, R, name):
    c, r = DC.filter_case(name), DC.restated_filter(name)
    eng = engine_of(gpu, c)
    before = snapshot(eng, c)
    got = eng.remove_floating_points(c.x, c.y, c.z, c.height_threshold, c.bin_size)
    assert_mask(got, r.keep, c.z)
    assert_untouched(eng, c, before)
    eng.close()


@pytest.mark.parametrize("name", ["bins_3", "cells_256", "tile_large", "moved"])
def test_floating_point_removal_of_device_tensors(gpu, R, name):
    import torch
    c, r = DC.filter_case(name), DC.restated_filter(name)
    eng = engine_of(gpu, c)
    d = [torch.from_numpy(np.array(v)).cuda() for v in (c.x, c.y, c.z)]
    before = snapshot(eng, c)
    got = eng.remove_floating_points(*d, c.height_threshold, c.bin_size)
    assert_mask(got.cpu().numpy().astype(bool), r.keep, c.z)
    for v, h in zip(d, (c.x, c.y, c.z)):                             # the cloud is read, not written
        assert np.array_equal(v.cpu().numpy().view(np.uint32), h.view(np.uint32))
    assert_untouched(eng, c, before)
    eng.close()


def test_moved_map_keeps_its_content(gpu, R):
    """The cell of a point on a map with a start index, and a map with content: nothing of it changes."""
    c, r = DC.filter_case("moved"), DC.restated_filter("moved")
    eng, ref = engine_of(gpu, c), DC.grid_of(c)
    ge, gr = eng.geometry(), ref.geometry()
    assert same_geometry(ge, gr) and ge.start_row != 0 and ge.start_col != 0 and gr.start_row != 0 and gr.start_col != 0
    rng = np.random.default_rng(7)
    content = rng.normal(0.0, 1.0, (ge.rows, ge.cols)).astype(F32)
    content[rng.uniform(size=content.shape) < 0.2] = np.nan
    eng.set_layer("elevation", content)
    eng.set_layer("elevation_max", content + F32(1.0))
    before = {k: eng.layer(k).copy() for k in eng.layers()}
    assert np.array_equal(before["elevation"].view(np.uint32), content.view(np.uint32))
    assert_mask(eng.remove_floating_points(c.x, c.y, c.z, c.height_threshold, c.bin_size), r.keep, c.z)
    assert eng.layers() == list(before) and same_geometry(eng.geometry(), gr)
    for k, v in before.items():
        assert np.array_equal(eng.layer(k).view(np.uint32), v.view(np.uint32)), k
    eng.close()


# ---- the whole pipeline ----
def build(gpu, p, on_device=False):
    arrays = dict(p.cloud)
    if on_device:
        import torch
        arrays = {k: torch.from_numpy(np.array(v.view(np.int32) if k == "rgb" else v)).cuda() for k, v in arrays.items()}
    return gpu.build_dem(arrays["x"], arrays["y"], arrays["z"], arrays["intensity"], arrays["rgb"],
                         config=gpu.DEMConfig(**p.config), return_stats=True)


def assert_dem(eng, st, n, dem, threshold=True):
    assert eng is not None and st["status"] == 0
    assert (st["n_input"], st["n_after_sor"], st["n_after_height"]) == (n, dem.n_after_sor, dem.n_after_height)
    if threshold:
        assert F32(st["sor_threshold"]).view(np.uint32) == F32(dem.threshold).view(np.uint32)
    if "n_points" in dem.store:
        assert st["n_points_used"] == int(dem.layer("n_points").sum())
        assert st["n_cells_written"] == int((dem.layer("n_points") > 0).sum())
    else:
        assert st["n_points_used"] == st["n_cells_written"] == 0
    g = eng.geometry()
    assert (g.length_x, g.length_y, g.resolution, g.position_x, g.position_y, g.rows, g.cols) == dem.geometry
    assert (g.start_row, g.start_col) == (0, 0)
    assert eng.layers() == dem.layers()
    assert_layers_bit_identical(eng, dem)


@pytest.mark.parametrize("name", DC.COMPARED)
def test_build_dem_at_the_limits(gpu, R, name):
    p, dem = DC.pipeline(name), DC.restated_pipeline(name)[0]
    eng, st = build(gpu, p)
    assert_dem(eng, st, p.cloud["x"].size, dem)
    if name in DC.NONE_SURVIVE:                                      # a map, not None: the three basic layers, all NaN
        assert st["n_after_height"] == 0 and eng.layers() == ["elevation", "elevation_min", "elevation_max"]
        assert all(np.isnan(eng.layer(k)).all() for k in eng.layers())
    if name == "fallback":
        assert st["n_sor_fallback"] >= 6, st                         # (tests/test_dem_restate.py: the six must be queued)
    eng.close()


@pytest.mark.parametrize("on_device", [False, True])
def test_build_dem_through_both_chunks_of_the_scan(gpu, R, on_device):
    p, dem = DC.pipeline("scan_chunks"), DC.restated_pipeline("scan_chunks")[0]
    eng, st = build(gpu, p, on_device)
    assert np.isfinite(st["sor_threshold"]) and st["n_after_sor"] == p.cloud["x"].size
    assert_dem(eng, st, p.cloud["x"].size, dem, threshold=False)
    eng.close()


def test_build_dem_refused_with_a_live_engine(gpu, R):
    """The height filter refuses the cloud after the map exists; the next call is served as if nothing had happened."""
    p = DC.pipeline("refused_late")
    with pytest.raises(gpu.EngineError):
        build(gpu, p)
    c, dem = TB.restated_dem("mean", True, 3)
    cfg = gpu.DEMConfig(method="mean", inpaint_iterations=3, **TB.CONFIG)
    eng, st = gpu.build_dem(c["x"], c["y"], c["z"], c["intensity"], c["rgb"], config=cfg, return_stats=True)
    assert_dem(eng, st, c["x"].size, dem)
    eng.close()
