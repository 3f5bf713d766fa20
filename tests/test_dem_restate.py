"""The NumPy restatement of buildDEM (tests/dem_restate.py) held to the reference's own answers: the four nanoPCL tests of
statisticalOutlierRemoval (lib/nanoPCL/tests/test_filters.cpp:386-458) and the five BuildDEMTest cases
(fastdem/tests/test_rasterization.cpp:344-429), plus the hand-checked corners of the histogram filter.  CPU only."""
import numpy as np
import pytest

import dem_restate as DR

F32 = np.float32


def lattice(nx, ny, nz=1):
    p = np.array([(x, y, z) for x in range(nx) for y in range(ny) for z in range(nz)], dtype=F32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def frange(lo, hi, step):
    """for (float v = lo; v <= hi; v += step): the accumulated fp32 values."""
    out, v = [], F32(lo)
    while v <= F32(hi):
        out.append(v)
        v = F32(v + F32(step))
    return out


def plane(lo, hi, step, z, skip=None):
    pts = [(x, y, F32(z)) for x in frange(lo, hi, step) for y in frange(lo, hi, step) if not (skip and skip(x, y))]
    p = np.array(pts, dtype=F32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


# ---- nanoPCL test_filters.cpp ----
def test_sor_all_inliers():                                          # :386-401
    keep, _, _ = DR.restate_sor(*lattice(3, 3, 3), 4, 3.0)
    assert keep.sum() == 27


def with_outlier(x, y, z):
    return np.append(x, F32(100)), np.append(y, F32(100)), np.append(z, F32(0))


def test_sor_basic():                                                # :403-422
    x, y, z = with_outlier(*lattice(5, 5))
    keep, mean, thr = DR.restate_sor(x, y, z, 4, 1.0)
    assert 24 <= keep.sum() < 26 and not keep[25]
    assert mean[12] == F32(1.0)                                      # an inner lattice point: four neighbours at 1


def test_sor_channel_preservation():                                 # :424-445
    x, y, z = with_outlier(*lattice(3, 3))
    keep, _, _ = DR.restate_sor(x, y, z, 3, 1.0)
    colours = np.array([i * 10 for i in range(9)] + [255])
    assert keep.sum() > 0 and colours[keep][0] < 200                 # the outlier's colour is not the first one


def test_sor_move_overload_keeps_the_inliers():                      # :447-458
    keep, _, _ = DR.restate_sor(*with_outlier(*lattice(5, 5)), 4, 1.0)
    assert keep.sum() >= 24


def test_sor_degenerate_inputs():                                    # :86-92
    e = np.zeros(0, dtype=F32)
    assert DR.restate_sor(e, e, e, 10)[0].size == 0
    one = np.ones(1, dtype=F32)
    assert not DR.restate_sor(one, one, one, 10)[0].any()
    assert not DR.restate_sor(*lattice(3, 3), 0)[0].any()
    assert DR.effective_k(11, 10) == 10 and DR.effective_k(5, 10) == 4 and DR.effective_k(5, -1) == 4
    two = DR.restate_sor(np.array([0, 1], dtype=F32), np.zeros(2, dtype=F32), np.zeros(2, dtype=F32), 10)
    assert two[0].all() and two[2] == F32(1.0)                       # both means 1, deviation 0


def test_duplicates_count_as_neighbours():
    x = np.array([0, 0, 0, 3], dtype=F32)
    zero = np.zeros(4, dtype=F32)
    mean = DR.knn_mean_distances(x, zero, zero, 2)
    assert list(mean) == [0.0, 0.0, 0.0, 3.0]


def test_threshold_sums_run_in_input_order():
    """np.cumsum is the sequential sum the reference's loops compute (np.sum is pairwise)."""
    rng = np.random.default_rng(3)
    mean = rng.uniform(0.01, 0.3, 5000).astype(F32)
    total = 0.0
    for v in mean:
        total += float(v)
    gm = total / mean.size
    ss = 0.0
    for v in mean:
        ss += (float(v) - gm) * (float(v) - gm)
    want = F32(F32(gm) + F32(F32(1.5) * F32(np.sqrt(ss / mean.size))))
    assert DR.sor_threshold(mean, 1.5) == want


# ---- findGroundPeak / removeFloatingPoints ----
def test_ground_peak_lowest_of_equal_peaks():
    z = np.array([0.05, 0.06, 1.05, 1.06, 0.55], dtype=F32)          # bins 0 and 10 hold two each, bin 5 one
    assert DR.restate_ground_peak(z, 0.1) == F32(F32(0.05) + F32(F32(0.5) * F32(0.1)))


def test_ground_peak_single_value_and_empty():
    assert DR.restate_ground_peak(np.array([2.0, 2.0, 2.0], dtype=F32), 0.1) == F32(F32(2.0) + F32(F32(0.5) * F32(0.1)))
    assert DR.restate_ground_peak(np.zeros(0, dtype=F32), 0.1) == 0.0


def test_ground_peak_refuses_a_bin_count_beyond_int():
    with pytest.raises(OverflowError):
        DR.restate_ground_peak(np.array([0.0, 3e9], dtype=F32), 1.0)


# ---- BuildDEMTest (test_rasterization.cpp:344-429) ----
def has_elevation_at(dem, px, py):
    ok, (r, c) = dem.grid.get_index(px, py)
    return ok and not np.isnan(dem.layer("elevation")[r, c]), (r, c)


def test_build_dem_empty_cloud_returns_uninitialized(R):             # :344-348
    e = np.zeros(0, dtype=F32)
    assert DR.restate_build_dem(R, e, e, e) is None


def test_build_dem_basic_pipeline(R):                                # :350-370
    dem = DR.restate_build_dem(R, *plane(-2.0, 2.0, 0.1, 0.0), resolution=0.5, sor_k=5, inpaint_iterations=0)
    assert dem is not None and "elevation" in dem.layers()
    has, (r, c) = has_elevation_at(dem, 0.0, 0.0)
    assert has and abs(dem.layer("elevation")[r, c] - 0.0) <= 0.1


def test_build_dem_inpainting_fills_holes(R):                        # :372-392
    gap = lambda x, y: abs(x) < F32(0.3) and abs(y) < F32(0.3)       # noqa: E731
    x, y, z = plane(-2.0, 2.0, 0.1, 1.0, skip=gap)
    assert has_elevation_at(DR.restate_build_dem(R, x, y, z, resolution=0.5, sor_k=5, inpaint_iterations=3), 0.0, 0.0)[0]


def test_build_dem_resolution_applied(R):                            # :394-407
    x, y, z = np.array([0, 1], dtype=F32), np.array([0, 1], dtype=F32), np.array([1, 2], dtype=F32)
    dem = DR.restate_build_dem(R, x, y, z, resolution=0.25, sor_k=1, inpaint_iterations=0)
    assert F32(dem.geometry[2]) == F32(0.25)


def test_build_dem_output_has_statistics_layers(R):                  # :409-429
    dem = DR.restate_build_dem(R, *plane(-1.0, 1.0, 0.2, 0.5), resolution=0.5, sor_k=3, inpaint_iterations=0)
    for name in ("elevation", "elevation_min", "elevation_max", "variance", "n_points"):
        assert name in dem.layers()


# ---- the helpers of tests/test_sor_edges_gpu.py and the clouds of tests/sor_cases.py ----
import sor_cases as SC  # noqa: E402


def test_knn_of_a_subset_equals_the_full_function():
    rng = np.random.default_rng(5)
    x, y, z = (rng.normal(0.0, s, 2000).astype(F32) for s in (4.0, 4.0, 0.3))
    x[100:103], y[100:103], z[100:103] = x[100], y[100], z[100]      # duplicates: only the query's own index is left out
    full = DR.knn_mean_distances(x, y, z, 10)
    pick = np.concatenate([[0, 1999, 100, 101], rng.permutation(2000)[:300]])
    for cells in (1 << 23, 2000 * 7):                                # one chunk, many chunks
        got = DR.knn_mean_distances_of(x, y, z, 10, pick, cells=cells)
        assert got.dtype == F32 and np.array_equal(got.view(np.uint32), full[pick].view(np.uint32))
    assert np.array_equal(DR.knn_mean_distances_of(x, y, z, 10, np.arange(2000)), full)


def test_knn_columns_round_twice_truncate_and_clamp():
    assert list(DR.knn_columns(np.array([0.0, 0.99, 1.0, 15.99, 16.0], dtype=F32), 0.0, 1.0, 17)) == [0, 0, 1, 15, 16]
    assert list(DR.knn_columns(np.array([16.0, 40.0, -3.0], dtype=F32), 0.0, 1.0, 16)) == [15, 15, 0]
    # h = 0.3: inv_h = fl(1 / fl(0.3)) and the product are rounded to fp32 (0.9 * inv_h is 2.9999998, not 3)
    p, inv = np.array([0.9, 1.2, 1.5], dtype=F32), F32(1.0) / F32(0.3)
    want = [int(F32(F32(v - F32(0.0)) * inv)) for v in p]
    assert list(DR.knn_columns(p, 0.0, 0.3, 100)) == want and want[0] == 2
    # a large common offset: the subtraction comes first and is exact
    q = np.array([400000.0, 400000.03125, 400002.5], dtype=F32)
    assert list(DR.knn_columns(q, 400000.0, 0.5, 100)) == [0, 0, 5]


def test_knn_within_rings_known_answers():
    # columns of 1 m over [0, 6] x [0, 1): the query at 2.5 with one point per column on its row
    x = np.array([2.5, 2.75, 1.5, 3.75, 0.25, 5.0, 6.0], dtype=F32)
    y = np.full(7, 0.5, dtype=F32)
    z = np.zeros(7, dtype=F32)
    g = (1.0, 0.0, 0.0, 7, 1)
    assert DR.knn_mean_within_rings(x, y, z, 1, 0, 0, *g) == F32(0.25)
    assert DR.knn_mean_within_rings(x, y, z, 2, 0, 0, *g) == np.inf               # one other point in its column
    assert DR.knn_mean_within_rings(x, y, z, 3, 0, 1, *g) == F32((0.25 + 1.0 + 1.25) / 3)
    assert DR.knn_mean_within_rings(x, y, z, 4, 0, 1, *g) == np.inf
    assert DR.knn_mean_within_rings(x, y, z, 4, 0, 2, *g) == F32((0.25 + 1.0 + 1.25 + 2.25) / 4)
    assert DR.knn_mean_within_rings(x, y, z, 4, 0, 6, *g) == DR.knn_mean_distances(x, y, z, 4)[0]
    # the query in the last column (the points at exactly max_x), rings clipped at the border
    assert DR.knn_mean_within_rings(x, y, z, 1, 6, 0, *g) == np.inf
    assert DR.knn_mean_within_rings(x, y, z, 1, 6, 1, *g) == F32(1.0)


def test_sor_grid_branches():
    assert DR.sor_grid(0, 0, 16, 16, 1024, 8) == (F32(1.0), 17, 17)               # tests/test_sor_gpu.py's `faces`
    assert DR.sor_grid(0, 0, 64, 64, 16384, 8) == (F32(1.0), 65, 65)
    assert DR.sor_grid(0, 0, 16, 16, 8192, 64) == (F32(1.0), 17, 17)              # per = k / 2
    assert DR.sor_grid(0, 0, 511.75, 0.0625, 4000, 8) == (F32(0.25), 2048, 1)     # the column cap binds: 0.179 < 0.25
    assert DR.sor_grid(0, 3, 16, 3, 300, 10) == (F32(5 * 16 / 300), 60, 1)        # no area: points per length
    assert DR.sor_grid(3, 0, 3, 16, 300, 10) == (F32(5 * 16 / 300), 1, 60)
    assert DR.sor_grid(-2.5, 7.25, -2.5, 7.25, 200, 10) == (F32(1.0), 1, 1)       # no extent: one column


@pytest.mark.parametrize("name", SC.DESIGNED)
def test_designed_probes_tell_a_search_that_stops_a_ring_early(name):
    c = SC.designed(name)
    rings = set()
    for p in c.probes:
        SC.check_probe(c, p)
        rings.add(p.ring)
    if name == "rings":
        assert rings == {0, 1, 2, 3, 4, 5}
    assert 5 in rings or name.endswith("a")                          # every bucket has a probe that must be queued


def test_whole_grid_exit_cloud_is_beyond_the_bound_of_ring_4():
    x, y, z, q = SC.whole_grid_exit()
    d2 = np.sort(((x - x[q]) ** 2 + (y - y[q]) ** 2) + (z - z[q]) ** 2)
    assert d2[1] > SC.lb2(4, 0.5) and (x[q], y[q]) == (4.5, 4.5)     # even the nearest point: the bound never stops it
    cx, cy = DR.knn_columns(x, 0.0, 1.0, 9), DR.knn_columns(y, 0.0, 1.0, 9)
    assert max(np.abs(cx - 4).max(), np.abs(cy - 4).max()) == 4      # ring 4 is the whole grid, ring 3 is not


def test_brute_force_clouds_reach_the_queue_by_the_grid_rule():
    for name, small in (("ends50+150", 50), ("ends30+70", 30)):
        x, y, z, k = SC.cloud(name)
        h, gx, gy = DR.sor_grid(x.min(), y.min(), x.max(), y.max(), x.size, k)
        assert gx >= 6 and gy == 1 and k == 64 > small - 1
        cx = DR.knn_columns(x, x.min(), h, gx)
        assert (cx[:small] == 0).all() and (cx[small:] >= 5).all()   # five columns from the small cluster: nothing
    x, y, z, k = SC.cloud("brute-sites")
    h, gx, gy = DR.sor_grid(x.min(), y.min(), x.max(), y.max(), x.size, k)
    assert 15.0 * 15.0 > float(SC.lb2(4, 0.5, h))                    # the tie's 15 m are beyond the bound of ring 4
    mean = DR.knn_mean_distances_of(x, y, z, k, np.arange(3000, x.size))
    assert (mean[:16] == 0).all() and (mean[16:21] > 10).all() and mean[21] == 15.0
