"""tests/raster_restate.py held to the reference's own known answers (fastdem/tests/test_rasterization.cpp, the
FromPointCloudTest / FromPointCloudStatsTest / ToPointCloudTest cases) and to the property that makes the GPU test
(tests/test_raster_gpu.py) see a wrong walk order: Welford's fp32 variance depends on the order of the points.  CPU only."""
import numpy as np

import raster_restate as RR

F32 = np.float32


class _Map:
    """A 10 x 10 m map at 0.5 m on the oracle's grid, with the layers of a fresh ElevationMap."""

    def __init__(self, R, width=10.0, height=10.0, res=0.5):
        self.grid = R.RefEngine(width, height, res)
        g = self.grid.geometry()
        self.order = list(RR.BASIC_LAYERS)
        self.layers = {n: np.full((g.rows, g.cols), np.nan, dtype=F32) for n in self.order}

    def run(self, pts, method="max", intensity=None, rgb=None):
        p = np.asarray(pts, dtype=F32).reshape(-1, 3)
        return RR.restate_raster(self.grid, self.layers, self.order, p[:, 0], p[:, 1], p[:, 2], intensity, rgb, method)

    def at(self, name, x, y):
        ok, (r, c) = self.grid.get_index(x, y)
        assert ok
        return self.layers[name][r, c]


def test_max_and_min_of_one_cell(R):
    m = _Map(R)
    m.run([(0.1, 0.1, 1.0), (0.15, 0.15, 5.0), (0.2, 0.2, 3.0)], "max")
    assert m.at("elevation", 0.1, 0.1) == F32(5.0) and m.at("elevation_min", 0.1, 0.1) == F32(1.0)
    assert m.at("elevation_max", 0.1, 0.1) == F32(5.0) and m.at("n_points", 0.1, 0.1) == F32(3.0)
    m2 = _Map(R)
    m2.run([(0.1, 0.1, 1.0), (0.15, 0.15, 5.0), (0.2, 0.2, 3.0)], "min")
    assert m2.at("elevation", 0.1, 0.1) == F32(1.0)
    m3 = _Map(R)
    m3.run([(0.1, 0.1, 1.0), (0.15, 0.15, 5.0), (0.2, 0.2, 3.0)], "minmax")
    assert m3.at("elevation", 0.1, 0.1) == F32(5.0)


def test_mean_of_two(R):
    m = _Map(R)
    m.run([(0.1, 0.1, 2.0), (0.15, 0.15, 4.0)], "mean")
    assert m.at("elevation", 0.1, 0.1) == F32(3.0)


def test_welford_sample_variance(R):
    m = _Map(R)
    written = m.run([(0.1, 0.1, 2.0), (0.15, 0.15, 4.0), (0.2, 0.2, 6.0)], "mean")
    assert m.at("elevation", 0.1, 0.1) == F32(4.0)
    assert m.at("variance", 0.1, 0.1) == F32(4.0) and m.at("n_points", 0.1, 0.1) == F32(3.0)
    assert written == ["elevation", "elevation_min", "elevation_max", "variance", "n_points"]
    assert m.order == RR.BASIC_LAYERS + ["variance", "n_points"]


def test_single_point(R):
    m = _Map(R)
    m.run([(1.0, 1.0, 7.0)])
    assert m.at("variance", 1.0, 1.0) == F32(0.0) and m.at("n_points", 1.0, 1.0) == F32(1.0)
    assert int(np.isfinite(m.layers["elevation"]).sum()) == 1   # untouched cells stay NaN


def test_nan_points_are_skipped(R):
    m = _Map(R)
    m.run([(0.1, 0.1, np.nan), (0.15, 0.15, 2.0), (0.2, 0.2, 4.0)])
    assert m.at("n_points", 0.1, 0.1) == F32(2.0)
    assert m.at("elevation_max", 0.1, 0.1) == F32(4.0) and m.at("elevation_min", 0.1, 0.1) == F32(2.0)


def test_intensity_is_written_and_the_layer_created(R):
    m = _Map(R)
    assert "intensity" not in m.layers
    m.run([(0.1, 0.1, 1.0)], intensity=np.array([0.7], dtype=F32))
    assert m.at("intensity", 0.1, 0.1) == F32(0.7)
    assert m.order[-1] == "intensity"
    # the first value wins unconditionally, then only a strictly greater one: a leading NaN stays
    m2 = _Map(R)
    m2.run([(0.1, 0.1, 1.0), (0.1, 0.1, 1.0)], intensity=np.array([np.nan, 3.0], dtype=F32))
    assert np.isnan(m2.at("intensity", 0.1, 0.1))


def test_colour_packing(R):
    m = _Map(R)
    m.run([(0.1, 0.1, 1.0)], rgb=np.array([(255 << 16) | (128 << 8) | 64], dtype=np.uint32))
    ok, (r, c) = m.grid.get_index(0.1, 0.1)
    assert m.layers["color"].view(np.uint32)[r, c] == 0x00FF8040
    cloud = RR.restate_to_cloud(m.layers, m.grid.geometry())
    assert cloud["rgb"].tolist() == [0x00FF8040] and cloud["intensity"] is None and cloud["z"].tolist() == [1.0]


def test_auto_size(R):
    x = np.array([-5.0, 5.0, 0.0], dtype=F32)
    y = np.array([-3.0, 3.0, 0.0], dtype=F32)
    lx, ly, res, px, py, rows, cols = RR.restate_auto_geometry(x, y, 0.5)
    assert abs(lx - 10.5) <= 0.5 and abs(ly - 6.5) <= 0.5 and res == 0.5 and (px, py) == (0.0, 0.0)
    grid = R.RefEngine(F32(10.5), F32(6.5), 0.5, position=(px, py))
    g = grid.geometry()
    assert (g.rows, g.cols, g.length_x, g.length_y) == (rows, cols, lx, ly)
    assert all(grid.get_index(float(a), float(b))[0] for a, b in zip(x, y))
    assert RR.restate_auto_geometry(np.zeros(0, F32), np.zeros(0, F32), 0.5) is None


def test_empty_cloud_is_no_map_change(R):
    m = _Map(R)
    assert m.run(np.zeros((0, 3), F32)) == [] and m.order == RR.BASIC_LAYERS
    assert m.run([(100.0, 100.0, 1.0)]) == [] and m.order == RR.BASIC_LAYERS     # outside: no cell, no layer


def test_to_cloud_of_an_empty_map_and_a_round_trip(R):
    m = _Map(R)
    assert RR.restate_to_cloud(m.layers, m.grid.geometry())["x"].size == 0
    m.run([(0.1, 0.1, 1.0), (2.1, -1.3, 2.0), (-3.2, 4.4, 3.0)], intensity=np.array([0.5, 0.25, 0.125], dtype=F32))
    cloud = RR.restate_to_cloud(m.layers, m.grid.geometry())
    assert cloud["x"].size == 3 and sorted(cloud["z"].tolist()) == [1.0, 2.0, 3.0]
    for x, y, z, a in zip(cloud["x"], cloud["y"], cloud["z"], cloud["intensity"]):   # cell centres land in their own cell
        assert m.at("elevation", float(x), float(y)) == z and m.at("intensity", float(x), float(y)) == a


def test_variance_depends_on_the_order():
    v = RR.order_sensitive_values()
    assert v.dtype == F32 and v.size == 4000
    _, var_a, n_a = RR.welford(v)
    _, var_b, n_b = RR.welford(v[::-1])
    assert n_a == n_b == 4000
    assert var_a.view(np.uint32) != var_b.view(np.uint32)
    assert abs(float(var_a) - float(var_b)) < 1e-3 * float(var_a)   # (the same variance, in other last bits)
