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
