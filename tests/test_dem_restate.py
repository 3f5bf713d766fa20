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


# ---- the clouds of tests/dem_cases.py: which path of the filter and of the compaction each one reaches.  What is shown
# here on the restatement alone, tests/test_dem_edges_gpu.py does not assert again ----
import dem_cases as DC  # noqa: E402
import test_build_dem_gpu as TB  # noqa: E402

# passes of the bin sort (keys 0 .. the largest bin index) and of the cell sort (keys 0 .. ncell, the skip key)
PASSES = {"bins_2": (2, 3), "bins_3": (3, 3), "bins_4": (4, 3), "cells_1": (1, 1), "cells_256": (2, 2), "cells_4": (1, 4),
          "long_run": (2, 2), "tile_large": (3, 2), "moved": (1, 2)}


def ncell_of(name):
    g = DC.grid_of(DC.filter_case(name)).geometry()
    return g.rows * g.cols


def test_sort_passes_follow_rs_key_bits():
    assert [DC.sort_passes(v) for v in (0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 32) - 1, 1 << 40)] == \
        [1, 1, 1, 2, 2, 3, 3, 4, 4, 4]


@pytest.mark.parametrize("name", DC.FILTER_CASES)
def test_filter_case_reaches_its_passes(R, name):
    c, r = DC.filter_case(name), DC.restated_filter(name)
    print(f"{name}: {c.x.size} points, {(r.key >= 0).sum()} with a cell, restated in {r.seconds:.2f} s")
    assert (DC.sort_passes(DC.largest_bin(name)), DC.sort_passes(ncell_of(name))) == PASSES[name]
    live = r.key >= 0
    assert 0.05 < r.keep[live].mean() < 0.95 and not r.keep[~live].any()


def test_cell_counts_at_the_edges_of_a_pass(R):
    assert ncell_of("cells_1") == 255 and ncell_of("cells_256") == 256 and ncell_of("cells_4") == 4097 * 4096 >= 1 << 24
    assert ncell_of("bins_2") == 260 * 260
    assert DC.sort_passes(256 - 1) == 1                              # what a sort sized for the cells alone would take


@pytest.mark.parametrize("name", DC.FILTER_CASES)
def test_grouped_restatement_equals_the_loop_on_the_filter_cases(R, name):
    c, r = DC.filter_case(name), DC.restated_filter(name)
    loop = DR.restate_floating(DC.grid_of(c), c.x, c.y, c.z, c.height_threshold, DC.bin_of(c))
    assert np.array_equal(loop, r.keep)


@pytest.mark.parametrize("height_threshold,bin_size", [(2.0, 0.0), (2.0, 0.25), (0.5, 0.0), (0.5, 0.03), (np.nan, 0.0)])
def test_grouped_restatement_equals_the_loop_on_the_first_filter_cloud(R, height_threshold, bin_size):
    x, y, z = TB.filter_cloud()
    grid = R.RefEngine(float(F32(TB.W)), float(F32(TB.H)), float(F32(TB.RES)))
    b = F32(bin_size) if bin_size > 0 else F32(TB.RES)
    assert np.array_equal(DR.restate_floating_grouped(grid, x, y, z, height_threshold, b),
                          DR.restate_floating(grid, x, y, z, height_threshold, b))


@pytest.mark.parametrize("name", DC.COMPARED)
def test_grouped_restatement_equals_the_loop_in_the_pipelines(R, name):
    a, b = DC.restated_pipeline(name)[0], DC.restated_pipeline(name, "loop")[0]
    assert (a.n_after_sor, a.n_after_height, a.geometry, a.layers()) == (b.n_after_sor, b.n_after_height, b.geometry, b.layers())
    for k in a.layers():
        assert np.array_equal(a.layer(k).view(np.uint32), b.layer(k).view(np.uint32)), k


def test_grouped_restatement_refuses_what_the_loop_refuses(R):
    grid = R.RefEngine(4.0, 3.0, 0.1)
    x = y = np.zeros(2, dtype=F32)
    for f in (DR.restate_floating, DR.restate_floating_grouped):
        with pytest.raises(OverflowError):
            f(grid, x, y, np.array([0.0, 3e9], dtype=F32), 2.0, F32(1.0))
        assert f(grid, x, y, np.array([0.0, 2e9], dtype=F32), 2.0, F32(1.0)).tolist() == [True, False]


def test_bin_sizes_give_different_masks_and_the_hand_made_cells_their_answers(R):
    masks = {n: DC.restated_filter(n).keep for n in DC.BIN_SIZES}
    assert all((masks[a] != masks[b]).any() for a in masks for b in masks if a < b)
    for name, keep in masks.items():
        c = DC.filter_case(name)
        m = c.marks
        assert list(c.z[m["tie_low_first"]]) == [0.5, 0.5, 30.0, 30.0, 10.0]          # the input order is the designed one
        assert list(c.z[m["tie_high_first"]]) == [30.0, 30.0, 0.5, 0.5, 10.0]
        assert keep[m["tie_low_first"]].tolist() == [True, True, False, False, False]
        assert keep[m["tie_high_first"]].tolist() == [False, False, True, True, False]
        at = m["cutoff_" + name]
        cut = DC.cutoff_of_zero(DC.BIN_SIZES[name], DC.BINS_HT)
        assert c.z[at[3]] == cut and c.z[at[4]] == np.nextafter(cut, F32(9)) and c.z[at[4]].dtype == F32
        assert keep[at].tolist() == [True, True, True, True, False]
        assert keep[m["single"]].all() and keep[m["all_equal"]].all() and keep[m["peak_high"]].all()
        assert keep[m["majority_low"]].sum() == 40 and keep[m["three_peaks"]].tolist() == [True, True] + [False] * 4
        assert keep[m["negative"]].tolist() == [True, True, False, False]
        assert keep[m["peak_inside"]].tolist() == [True] * 5 + [False]
        for idx in m.values():                                       # every hand-made cell is a cell of its own
            assert len(set(DC.restated_filter(name).key[idx])) == 1
        assert np.isnan(c.z[-2:]).all() and (DC.restated_filter(name).key[-4:] == -1).all()


def test_cells_256_puts_skipped_points_between_the_points_of_storage_cell_0(R):
    c, r = DC.filter_case("cells_256"), DC.restated_filter("cells_256")
    cell0 = np.flatnonzero(r.key == DC.cell_key(0, 0))
    early, high = c.marks["cell0_early"], c.marks["cell0_high"]
    assert np.array_equal(cell0, np.concatenate([early, high]))
    between = np.arange(early[-1] + 1, high[0])
    assert (r.key[between] == -1).sum() >= 50 and np.isin(c.marks["skipped"], between).all()
    assert (r.key[c.marks["skipped"]] == -1).all()
    assert np.isnan(c.z[between]).sum() == 30                        # half without a z, half outside the map
    live, group, z_min, bins = DR.floating_bins(r.key, c.z, DC.bin_of(c))
    b0 = bins[np.isin(live, cell0)]
    assert np.unique(b0).size == 501 and np.bincount(b0).max() == 5 == (b0 == 0).sum()
    assert r.keep[early].all() and not r.keep[high].any()            # the peak is bin 0: all thousand go
    # the run of the thousand alone has its peak in bin 10: a cutoff of 1.55 m would keep the first dozen of them
    assert np.bincount(b0[5:]).argmax() == 10 and (c.z[high] <= 1.55).sum() == 12


def test_long_run_has_its_two_cells(R):
    c, r = DC.filter_case("long_run"), DC.restated_filter("long_run")
    a = np.flatnonzero(r.key == DC.cell_key(*DC.LONG_CELL))
    b = np.flatnonzero(r.key == DC.cell_key(*DC.ONE_BIN_CELL))
    assert a.size == 5000 and b.size == 1025
    assert np.array_equal(a, c.marks["long"]) and np.array_equal(b, c.marks["one_bin"])
    live, group, z_min, bins = DR.floating_bins(r.key, c.z, DC.bin_of(c))
    count = np.bincount(bins[np.isin(live, a)])
    assert (count > 0).sum() == 410 >= 300 and np.flatnonzero(count == count.max()).tolist() == [5, 350]
    assert np.unique(bins[np.isin(live, b)]).size == 1
    cut = F32(F32(F32(0.0) + F32(F32(5.5) * F32(0.01))) + F32(0.5))
    assert np.array_equal(r.keep[a], c.z[a] <= cut) and 500 < r.keep[a].sum() < 1000   # the low peak is the ground
    assert r.keep[b].all()
    # in the input the two cells' points and the others' alternate: no stretch of 256 inputs is one cell's alone
    other = r.key != DC.cell_key(*DC.LONG_CELL)
    runs = np.diff(np.flatnonzero(np.r_[True, other, True]))
    assert runs.max() < 64 and a[-1] - a[0] > 7000 and b[-1] - b[0] > 7000


def test_tile_large_is_beyond_the_small_tile(R):
    c, r = DC.filter_case("tile_large"), DC.restated_filter("tile_large")
    assert c.x.size == 600_001 > 600_000 and (r.key >= 0).sum() == 20_000 == (~np.isnan(c.z)).sum()


def test_moved_map_has_a_start_index(R):
    c, r = DC.filter_case("moved"), DC.restated_filter("moved")
    g = DC.grid_of(c).geometry()
    assert g.start_row != 0 and g.start_col != 0 and (g.rows, g.cols) == (40, 30)
    for name, idx in c.marks.items():
        assert len(set(r.key[idx])) == 1 and r.keep[idx].tolist() == [True] * 46 + [False, False], name
    assert {DC.cell_key(0, 0), DC.cell_key(39, 29), DC.cell_key(g.start_row, g.start_col)} <= set(r.key)
    assert (r.key[-2:] == -1).all()


def test_none_survives_and_the_reference_returns_the_bare_map(R):
    for name in DC.NONE_SURVIVE:
        dem = DC.restated_pipeline(name)[0]
        assert dem is not None and dem.n_after_height == 0 < dem.n_after_sor
        assert dem.layers() == ["elevation", "elevation_min", "elevation_max"]
        assert all(np.isnan(dem.layer(k)).all() for k in dem.layers()) and dem.geometry[5:] == (31, 21)
    few = DC.restated_pipeline("minus_one_metre")[0]
    assert 0 < few.n_after_height < 64                               # less than one wavefront of survivors


def test_odd_geometries(R):
    assert DC.restated_pipeline("one_cell")[0].geometry[5:] == (1, 1)
    assert DC.restated_pipeline("one_row")[0].geometry[5:] == (1, 41)
    p, dem = DC.pipeline("utm"), DC.restated_pipeline("utm")[0]
    assert dem.geometry[3:5] == (5.0e5, 4.9e6) and np.unique(p.cloud["y"]).size < 200   # fp32 steps of 0.5 m in y
    keep = DR.restate_sor(p.cloud["x"], p.cloud["y"], p.cloud["z"], p.config["sor_k"], p.config["sor_std_mul"])[0]
    key = DR.floating_cells(dem.grid, p.cloud["x"][keep], p.cloud["y"][keep], p.cloud["z"][keep])
    print(f"utm: {(key < 0).sum()} of {key.size} survivors of the outlier removal have no cell")
    for name in ("one_cell", "one_row", "utm"):
        d = DC.restated_pipeline(name)[0]
        assert 0 < d.n_after_height < d.n_after_sor < DC.pipeline(name).cloud["x"].size


def test_scan_chunks_has_more_than_1024_blocks_in_both_compactions(R):
    p = DC.pipeline("scan_chunks")
    dem, seconds = DC.restated_pipeline("scan_chunks")
    print(f"scan_chunks restated in {seconds:.1f} s")
    n = p.cloud["x"].size
    assert n == DC.N_SCAN_CHUNKS >= 262_145 + 256 and dem.n_after_sor == n
    assert -(-n // 256) > 1024 and -(-dem.n_after_sor // 256) > 1024
    gone = 1.0 - dem.n_after_height / dem.n_after_sor
    assert 0.10 < gone < 0.40, gone
    assert p.config["sor_std_mul"] == 1e9 and np.sqrt(n) < 1e9       # the docstring's argument: every point passes SOR


def test_refused_late_is_refused_by_the_height_filter_and_not_before(R):
    p = DC.pipeline("refused_late")
    c = p.cloud
    keep, _, thr = DR.restate_sor(c["x"], c["y"], c["z"], p.config["sor_k"], p.config["sor_std_mul"])
    assert keep.all() and np.isfinite(thr) and c["z"][-1] == F32(3e9)
    with pytest.raises(OverflowError):
        DC.restated_pipeline("refused_late")


def test_fallback_cloud_reaches_the_queue_by_the_grid_rule(R):
    p = DC.pipeline("fallback")
    n = p.cloud["x"].size
    assert DC.sor_must_queue(p.cloud, p.config["sor_k"], np.arange(n - 6, n)) == 6
    keep = DR.restate_sor(p.cloud["x"], p.cloud["y"], p.cloud["z"], p.config["sor_k"], p.config["sor_std_mul"])[0]
    assert not keep[-6:].any() and DC.restated_pipeline("fallback")[0].geometry[5:] == (31, 21)
