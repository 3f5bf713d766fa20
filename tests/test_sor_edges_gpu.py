"""The outlier removal's k-NN search (fastdem_amd/csrc/fdm_knn.hpp, the grid rule sor_grid in fdm_engine_dem.inl) where
its stopping rule, its brute-force queue and its grid rule can go wrong — the clouds of tests/sor_cases.py against the
brute-force restatement of tests/dem_restate.py.  The contract is tests/test_sor_gpu.py's: the per-point mean distances
and the threshold bit for bit, the keep mask equal; tolerance 0 everywhere.

  designed probes   a query whose true k-th neighbour lies one ring beyond a farther decoy: rings 0 .. 4 and the queue,
                    the four faces, margins of 1/64, 1/4 and 31/64, border and corner columns with clipped rings, the
                    k-th distance on either side of the bound; a reduced set for k = 4, 5, 16, 17, 32, 33 and 64 (every
                    top-k bucket of k_knn_search and of k_knn_brute at both of its edges); the whole-cloud exit
  k_knn_brute       a cloud of 200 (and of 100) points that still queues, lanes with two, one or no candidate; queued
                    duplicates; a queued query whose k nearest are equidistant
  sor_grid          the 2 048-column cap, boxes without area (two lines, a pole, one point repeated), two dense corners
  scale             a UTM-like offset, powers of two, 700 001 points (512 sampled queries — the one place where less than
                    every mean is compared to brute force — and the engine's own threshold and mask re-derived)

Every case first asserts, on the restatement alone, that no mean distance lies within 16 ulp of the threshold (one point
repeated: every mean and the threshold are exactly 0, nothing can flip; the 700 001 points: the mask is held to the
engine's own means and threshold instead).  A path a case relies on — the queue, the cap, the grid, the column size — is
asserted from sor_last_stats(), never assumed.

Power-of-two scaling is exact only while nothing underflows.  The denormal and the overflow regime are out of scope:
2^50 and 2^-40 leave every product of the `arbitrary` cloud normal and the means must be the unscaled means times the
factor at every point; at 2^-60 the squares of differences below 2^-3 m are denormal, the restatement itself departs
from the scaled means at 8 of the 2 000 points, and the scaling identity is asserted at the others (the bits against the
restatement at all of them).

Run on the GPU box:  python -m pytest tests/test_sor_edges_gpu.py -m gpu
"""
import functools

import numpy as np
import pytest

import dem_restate as DR
import sor_cases as SC

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def restate(x, y, z, k, std_mul, what):
    """restate_sor with the 16 ulp rule asserted; the arrays read-only."""
    keep, mean, thr = DR.restate_sor(x, y, z, k, std_mul)
    gap = DR.ulp_gap_to_threshold(mean, thr)
    print(f"{what} k={k}: threshold {thr!r}, nearest mean {gap:.3g} ulp away, {int(keep.sum())} of {x.size} kept")
    # (one point repeated: every distance is 0, both sums are 0, nothing rounds — the gap is 0 by construction)
    assert gap >= 16 or (what == "one-point" and thr == 0 and not mean.any()), (what, k, gap)
    for a in (keep, mean):
        a.setflags(write=False)
    return keep, mean, thr


@functools.lru_cache(maxsize=None)
def restated_designed(name):
    c = SC.designed(name)
    for p in c.probes:                                               # before any GPU call: every probe discriminates
        SC.check_probe(c, p)
    return (c,) + restate(*c.xyz(), c.k, 1.0, name)


@functools.lru_cache(maxsize=None)
def restated_named(name, scale_exp=0):
    x, y, z, k = SC.cloud(name)
    f = F32(2.0) ** scale_exp
    x, y, z = x * f, y * f, z * f                                    # exact: a power of two, every coordinate stays normal
    assert np.isfinite(np.stack([x, y, z])).all() and (np.abs(x[x != 0]) >= 2.0 ** -100).all()
    return (x, y, z, k) + restate(x, y, z, k, 1.0, f"{name}*2^{scale_exp}" if scale_exp else name)


def run(gpu, x, y, z, k, keep, mean, thr):
    """One call held to the restatement; returns the call's stats and its means."""
    got_keep, got_mean, got_thr = gpu.statistical_outlier_removal(x, y, z, k, 1.0, return_details=True)
    st = gpu.sor_last_stats()
    bad = np.flatnonzero(bits(got_mean) != bits(mean))
    assert bad.size == 0, (f"{bad.size} mean distances differ, e.g. point {bad[0]} at ({x[bad[0]]!r}, {y[bad[0]]!r}, "
                           f"{z[bad[0]]!r}): {got_mean[bad[0]]!r} vs {mean[bad[0]]!r}; {st}")
    assert bits(got_thr) == bits(thr), (got_thr, thr)
    assert np.array_equal(got_keep, keep)
    assert st["n_queries"] == x.size and 0 <= st["n_fallback"] <= x.size
    h, gx, gy = DR.sor_grid(x.min(), y.min(), x.max(), y.max(), x.size, k)
    assert (bits(st["voxel"]), st["grid_x"], st["grid_y"]) == (bits(h), gx, gy), (st, h, gx, gy)
    print({a: b for a, b in st.items() if a != "ms"})
    return st, got_mean


# ---- 1. the stopping rule ----
@pytest.mark.parametrize("name", SC.DESIGNED)
def test_designed_probes(gpu, name):
    c, keep, mean, thr = restated_designed(name)
    st, got = run(gpu, *c.xyz(), c.k, keep, mean, thr)
    assert st["voxel"] == 1.0 and (st["grid_x"], st["grid_y"]) == (c.E + 1, c.E + 1), st
    for p in c.probes:
        assert bits(got[p.index]) == bits(mean[p.index]), p          # (covered by run(): named here)
    queued = sum(p.ring == 5 for p in c.probes)
    # the fillers are dense (a point in every filler column at least): only a probe's own points can be queued
    assert queued <= st["n_fallback"] <= sum(len(p.points(c.k, c.E)) for p in c.probes), st
    if not name.endswith("a"):
        assert st["n_fallback"] >= 1, st                             # this bucket's k_knn_brute ran


def test_whole_cloud_exit_at_ring_4(gpu):
    x, y, z, q = SC.whole_grid_exit()
    keep, mean, thr = restate(x, y, z, 8, 1.0, "whole-grid-exit")
    st, got = run(gpu, x, y, z, 8, keep, mean, thr)
    assert st["voxel"] == 1.0 and (st["grid_x"], st["grid_y"]) == (9, 9), st
    assert st["n_fallback"] == 0, st                                 # the centre is beyond the bound of ring 4: the exit took it
    assert got[q] == mean[q] and mean[q] > 4.5


# ---- 2. k_knn_brute at its edges ----
@pytest.mark.parametrize("name,small", [("ends50+150", 50), ("ends30+70", 30)])
def test_small_cloud_that_still_queues(gpu, name, small):
    x, y, z, k, keep, mean, thr = restated_named(name)
    st, _ = run(gpu, x, y, z, k, keep, mean, thr)
    assert k == 64 and st["grid_x"] >= 6 and st["grid_y"] == 1, st
    assert small <= st["n_fallback"] <= x.size, st                   # every query of the small cluster, at the least


def test_queued_duplicates_and_ties(gpu):
    x, y, z, k, keep, mean, thr = restated_named("brute-sites")
    st, got = run(gpu, x, y, z, k, keep, mean, thr)
    assert st["n_fallback"] >= 6, st                                 # the five copies and the centre of the sphere
    assert not got[3000:3016].any()                                  # k + 5 copies and the point itself: exactly 0
    assert (got[3016:3021] == got[3016]).all() and got[3016] > 10    # five copies: the same k nearest, four of them at 0
    assert got[3021] == 15.0                                         # thirty equidistant neighbours, k = 10 of them taken


# ---- 3. the grid rule's branches ----
def test_column_cap(gpu):
    x, y, z, k, keep, mean, thr = restated_named("strip")
    st, _ = run(gpu, x, y, z, k, keep, mean, thr)
    assert (st["grid_x"], st["grid_y"], st["voxel"]) == (2048, 1, 0.25), st
    cx = DR.knn_columns(x, x.min(), 0.25, 2048)
    assert (cx == 0).sum() >= 8 and (cx == 2047).sum() == 8 and (cx == 2046).sum() >= 8 and (x[cx == 2047] == x.max()).all()


@pytest.mark.parametrize("name,grid,voxel", [("line-x", (60, 1), F32(5 * 16 / 300)), ("line-y", (1, 60), F32(5 * 16 / 300)),
                                             ("pole", (1, 1), 1.0), ("one-point", (1, 1), 1.0)])
def test_boxes_without_area(gpu, name, grid, voxel):
    x, y, z, k, keep, mean, thr = restated_named(name)
    st, got = run(gpu, x, y, z, k, keep, mean, thr)
    assert (st["grid_x"], st["grid_y"]) == grid and st["voxel"] == voxel, st
    if name == "one-point":
        assert not got.any() and thr == 0 and keep.all()


def test_two_dense_corners(gpu):
    x, y, z, k, keep, mean, thr = restated_named("two-corners")
    st, _ = run(gpu, x, y, z, k, keep, mean, thr)
    cx, cy = DR.knn_columns(x, x.min(), st["voxel"], st["grid_x"]), DR.knn_columns(y, y.min(), st["voxel"], st["grid_y"])
    occupied = np.unique(cy * st["grid_x"] + cx).size
    assert st["grid_x"] * st["grid_y"] > 500 and occupied <= 8, (st, occupied)   # everything in a few long runs


# ---- 4. scale ----
def test_utm_like_offsets(gpu):
    x, y, z, k, keep, mean, thr = restated_named("utm")
    assert x.min() >= 4.0e5 and y.min() >= 5.0e6 and np.unique(y).size <= 121    # y sits on a lattice of 1/2 m
    run(gpu, x, y, z, k, keep, mean, thr)


@pytest.mark.parametrize("scale_exp", [-60, -40, 50])
def test_power_of_two_scaling(gpu, scale_exp):
    x0, y0, z0, k, keep0, mean0, thr0 = restated_named("arbitrary")
    x, y, z, _, keep, mean, thr = restated_named("arbitrary", scale_exp)
    f = F32(2.0) ** scale_exp
    exact = mean == mean0 * f                                        # on the restatement alone: no underflow behind this mean
    assert exact.all() if scale_exp != -60 else exact.sum() >= 0.99 * exact.size, int((~exact).sum())
    _, got0 = run(gpu, x0, y0, z0, k, keep0, mean0, thr0)
    _, got = run(gpu, x, y, z, k, keep, mean, thr)
    assert np.array_equal(bits(got[exact]), bits((got0 * f)[exact]))


@functools.lru_cache(maxsize=None)
def big_case():
    x, y, z = SC.big_cloud()
    sample = SC.big_sample(x, y)
    assert sample.size >= SC.BIG_SAMPLE and {0, SC.BIG_N - 1, *SC.BIG_PLANTED} <= set(sample.tolist())
    want = DR.knn_mean_distances_of(x, y, z, SC.BIG_K, sample)
    assert (want[np.isin(sample, SC.BIG_PLANTED)] > 20).all() and np.median(want) < 1
    return x, y, z, sample, want


def test_700001_points_from_device_arrays(gpu):
    import torch
    x, y, z, sample, want = big_case()
    d = [torch.from_numpy(v).cuda() for v in (x, y, z)]
    got_keep, got_mean, got_thr = gpu.statistical_outlier_removal(*d, SC.BIG_K, 1.0, return_details=True)
    st = gpu.sor_last_stats()
    got_mean, got_keep = got_mean.cpu().numpy(), got_keep.cpu().numpy().astype(bool)
    print({a: b for a, b in st.items() if a != "ms"})
    bad = np.flatnonzero(bits(got_mean[sample]) != bits(want))
    assert bad.size == 0, (bad.size, sample[bad[0]], got_mean[sample[bad[0]]], want[bad[0]], st)
    assert bits(got_thr) == bits(DR.sor_threshold(got_mean, 1.0)), got_thr
    assert np.array_equal(got_keep, got_mean <= got_thr)
    assert not got_keep[list(SC.BIG_PLANTED)].any()
    h, gx, gy = DR.sor_grid(x.min(), y.min(), x.max(), y.max(), x.size, SC.BIG_K)
    assert (bits(st["voxel"]), st["grid_x"], st["grid_y"]) == (bits(h), gx, gy), (st, h, gx, gy)
    assert st["n_queries"] == SC.BIG_N and len(SC.BIG_PLANTED) <= st["n_fallback"] < SC.BIG_N // 100, st
