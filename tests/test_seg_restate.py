"""CPU checks of the segmentation restatement (tests/seg_restate.py), of the case table the GPU test uses
(tests/seg_cases.py), and of the engine's host algebra (fastdem_amd/csrc/fdm_segment_host.hpp), which is compiled alone
into a sanitized stand-alone program and run as a child process.

The restatement is held to every assertion of nanoPCL's RANSAC, ground and boundary tests (tests/test_segmentation.cpp
:283-376, :382-498, :511-549; line numbers below are that file's) — on the rand-free clouds as they are, on seeded clouds
of the same construction where the reference draws from rand().  ADMISSION: a plane case is in the table only if its
refined coefficients and final inlier list are identical under the three summation orders and both eigen-solvers, and
if log(1 - p) / log(1 - w^3) at every best-update is no closer than 1e-9 to an integer.  Every case must be admitted.

The large cases (tests/seg_cases_large.py) and the wide ones of the small table are held to the same admission and to
SENSITIVITY: each exists to reach one branch that only size reaches, and the restatement of the computation with that
branch skipped must give another observable answer — else the case could not fail for it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import seg_cases as SC
import seg_cases_large as SL
import seg_restate as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the reference's own tests ----
def ground_plane(seed, nx, ny, spacing, noise=0.01):  # createGroundPlane (:31-40), seeded
    rng = np.random.default_rng(seed)
    pts = [(x * spacing, y * spacing, float(rng.integers(0, 100)) * noise * 0.01) for x in range(nx) for y in range(ny)]
    return SC._xyz(pts)


def test_ransac_plane_detection():  # :283-290
    r = SR.segment_plane(*ground_plane(1, 20, 20, 0.5), distance_threshold=0.05)
    assert r["success"] and r["fitness"] > 0.9


def test_ransac_plane_model_accuracy():  # :292-307
    r = SC.plane_answer("grid_z1")
    assert r["success"]
    assert abs(abs(r["coefficients"][2]) - 1.0) < 0.01 and abs(abs(r["coefficients"][3]) - 1.0) < 0.1
    assert r["iterations"] == 1000 and r["inliers"].size == 100 and r["fitness"] == 1.0
    assert 0 in r["valid"], "the grid's samples include collinear ones"


def test_ransac_inlier_outlier_split():  # :309-324
    x, y, z = ground_plane(2, 10, 10, 1.0)
    ex = SC._xyz([(float(i % 10), float(i // 10), 5.0) for i in range(20)])
    x, y, z = np.concatenate([x, ex[0]]), np.concatenate([y, ex[1]]), np.concatenate([z, ex[2]])
    r = SR.segment_plane(x, y, z, distance_threshold=0.1)
    out = SR.outliers(r["inliers"], x.size)
    assert r["success"] and r["inliers"].size >= 100 * 0.9 and out.size >= 15
    assert np.array_equal(np.sort(np.concatenate([r["inliers"], out])), np.arange(x.size))


def test_ransac_multiple_planes():  # :326-350
    res = SC.multi_answer("two_planes")
    assert len(res) >= 2
    assert all(r["inliers"].size == 100 for r in res[:2])
    assert not set(res[0]["inliers"].tolist()) & set(res[1]["inliers"].tolist())


def test_ransac_collinear_points():  # :352-364
    r = SC.plane_answer("line10")
    assert r["inliers"].size <= 10
    assert not r["success"] and r["iterations"] == 0 and r["valid"] == [0] * 100  # every sample is collinear


def test_ransac_plane_from_points():  # :366-376
    m, valid = SR.plane_from_points((0, 0, 0), (1, 0, 0), (0, 1, 0))
    assert valid and abs(abs(m[2]) - 1.0) < 0.01 and abs(m[3]) < 0.01
    assert not SR.plane_from_points((0, 0, 0), (1, 0, 0), (2, 0, 0))[1]
    assert not SR.plane_from_points((0, 0, 0), (np.nan, 0, 0), (0, 1, 0))[1]


def ground_with_obstacles(seed):  # createGroundWithObstacles (:78-105), seeded
    rng = np.random.default_rng(seed)
    r = lambda: float(rng.integers(0, 100))  # noqa: E731
    pts = [(x * 0.5 + r() * 0.004, y * 0.5 + r() * 0.004, r() * 0.001)
           for x in range(-10, 11) for y in range(-10, 11) for _ in range(3)]
    pts += [(2.0 + r() * 0.005, 2.0 + r() * 0.005, 1.0 + r() * 0.01) for _ in range(40)]
    pts += [(-2.0 + r() * 0.005, -2.0 + r() * 0.005, 1.0 + r() * 0.01) for _ in range(40)]
    return SC._xyz(pts)


def dense_layer(rng, nx, ny, per, z, x0=0.0):
    r = lambda: float(rng.integers(0, 100))  # noqa: E731
    return [(x0 + x + r() * 0.004, y + r() * 0.004, z) for x in range(nx) for y in range(ny) for _ in range(per)]


def test_ground_basic_segmentation():  # :382-391
    cloud = ground_with_obstacles(3)
    g, o = SR.segment_ground(*cloud, grid_resolution=0.5, ground_thickness=0.3, max_ground_height=0.5)
    assert g.size > 0 and o.size > 0 and g.size + o.size == cloud[0].size


def test_ground_grid_resolution():  # :393-418
    rng = np.random.default_rng(4)
    r = lambda: float(rng.integers(0, 100))  # noqa: E731
    pts = [(x * 0.5 + r() * 0.004, y * 0.5 + r() * 0.004, r() * 0.001) for x in range(20) for y in range(20) for _ in range(3)]
    pts += [(5.0, 5.0, 1.0 + i * 0.05) for i in range(20)]
    cloud = SC._xyz(pts)
    assert SR.segment_ground(*cloud, grid_resolution=0.5)[0].size > 0
    assert SR.segment_ground(*cloud, grid_resolution=2.0)[0].size > 0


def test_ground_thickness_config():  # :420-460
    rng = np.random.default_rng(5)
    cloud = SC._xyz(dense_layer(rng, 10, 5, 5, 0.0) + dense_layer(rng, 10, 5, 3, 0.2))
    thin = SR.segment_ground(*cloud, ground_thickness=0.1, grid_resolution=1.0)
    thick = SR.segment_ground(*cloud, ground_thickness=0.5, grid_resolution=1.0)
    assert thick[0].size > thin[0].size


def test_ground_height_config():  # :462-498
    rng = np.random.default_rng(6)
    cloud = SC._xyz(dense_layer(rng, 10, 5, 3, 0.0) + dense_layer(rng, 10, 5, 3, 1.0, x0=20.0))
    g, o = SR.segment_ground(*cloud, max_ground_height=0.5, grid_resolution=1.0)
    assert g.size > 0 and o.size > 0
    assert np.array_equal(g, np.arange(150)) and np.array_equal(o, np.arange(150, 300))


def test_boundary_conditions():  # :511-549
    for name in ("zero_points", "one_point", "two_points"):
        r = SC.plane_answer(name)
        assert not r["success"] and r["iterations"] == 0 and r["inliers"].size == 0
        assert np.array_equal(r["coefficients"], np.array([0, 0, 1, 0], dtype=F))
    g, o = SR.segment_ground(*SC._xyz([]))
    assert g.size == 0 and o.size == 0
    g, o = SC.ground_answer("n1")
    assert g.size + o.size == 1


# ---- the case table ----
@pytest.mark.parametrize("name", sorted(SC.plane_cases()))
def test_plane_case_is_admitted(name):
    base = SC.plane_answer(name)
    for order in ("forward", "reversed", "pairwise"):
        for solver in ("eigh", "jacobi"):
            r = SC.plane_answer(name, order, solver)
            assert np.array_equal(r["coefficients"].view(np.uint32), base["coefficients"].view(np.uint32)), (order, solver)
            assert np.array_equal(r["inliers"], base["inliers"]), (order, solver)
            assert (r["iterations"], r["success"]) == (base["iterations"], base["success"])
    for q in base["quotients"]:
        assert abs(q - round(q)) >= 1e-9, q
    idx = SC.plane_cases()[name][1].get("indices")
    n_list = SC.plane_cases()[name][0][0].size if idx is None else idx.size
    assert base["fitness"] == base["inliers"].size / float(n_list) if n_list else base["fitness"] == 0.0


@pytest.mark.parametrize("name", sorted(SC.multi_cases()))
def test_multi_case_is_admitted(name):
    base = SC.multi_answer(name)
    for order in ("forward", "reversed", "pairwise"):
        for solver in ("eigh", "jacobi"):
            res = SC.multi_answer(name, order, solver)
            assert len(res) == len(base)
            for r, b in zip(res, base):
                assert np.array_equal(r["coefficients"].view(np.uint32), b["coefficients"].view(np.uint32))
                assert np.array_equal(r["inliers"], b["inliers"]) and r["iterations"] == b["iterations"]
    for b in base:
        for q in b["quotients"]:
            assert abs(q - round(q)) >= 1e-9, q


def test_plane_cases_cover_what_the_table_promises():
    B = SC.BATCH
    its = {name: SC.plane_answer(name)["iterations"] for name in SC.plane_cases()}
    print(its)
    for name in SC.WITHIN_ONE_BATCH:
        assert 0 < its[name] <= B, (name, its[name])
    for name in SC.ACROSS_BATCH_EDGES:
        cap = SC.plane_cases()[name][1].get("max_iterations", 1000)
        assert 2 * B < its[name] < cap, (name, its[name])
    for name in SC.AT_THE_CAP:
        assert its[name] == SC.plane_cases()[name][1].get("max_iterations", 1000), (name, its[name])
    assert SC.plane_cases()["scene30_cap100"][1]["max_iterations"] % B != 0
    # the scenes' planes are found: about the share of points the scene was built with
    for name, share in (("scene45", 0.45), ("scene30", 0.30), ("scene20", 0.20), ("scene12", 0.12), ("scene70k", 0.5)):
        r = SC.plane_answer(name)
        assert r["success"] and share - 0.02 <= r["fitness"] <= share + 0.06, (name, r["fitness"])
    # the list of every third point: positions are sampled, the duplicate is reported twice
    r = SC.plane_answer("scene45_third")
    idx = SC.plane_cases()["scene45_third"][1]["indices"]
    assert r["success"] and set(r["inliers"].tolist()) <= set(idx.tolist())
    assert np.count_nonzero(r["inliers"] == idx[6]) in (0, 2)
    # NaN / inf points are sampled (invalid models) and never inliers
    r = SC.plane_answer("scene45_nan_inf")
    assert r["success"] and not set(r["inliers"].tolist()) & {3, 10, 17, 40, 41}
    # min_inliers above the best count: the default result, iterations 0
    r = SC.plane_answer("scene45_min_inliers")
    assert not r["success"] and r["iterations"] == 0 and r["loop_iterations"] > 0
    # refinement off: the sample's model is returned
    r = SC.plane_answer("scene45_unrefined")
    assert np.array_equal(r["coefficients"], r["unrefined"]) and r["moments"] is None
    with pytest.raises(ValueError):
        SR.segment_plane(*SC.INDEX_ERROR[0], **SC.INDEX_ERROR[1])
    # three planes: the third is below min_fitness and is not returned
    res = SC.multi_answer("three_planes")
    assert len(res) == 2 and res[0]["fitness"] > 0.4 and 0.1 <= res[1]["fitness"]


def test_sign_rule():
    c = np.array([1.0, 2.0, 3.0])
    up = SR.refined_model(np.array([0.0, 0.6, 0.8]), c, np.array([0, 0, 1], dtype=F))
    down = SR.refined_model(np.array([0.0, -0.6, -0.8]), c, np.array([0, 0, 1], dtype=F))
    assert np.array_equal(up, down) and up[2] > 0  # (as values: the flip turns the zero component into -0.0)
    flipped = SR.refined_model(np.array([0.0, 0.6, 0.8]), c, np.array([0, 0, -1], dtype=F))
    assert np.array_equal(flipped[:3], -up[:3]) and flipped[3] == -up[3]
    # a dot of exactly 0: the first non-zero component is positive
    tie = SR.refined_model(np.array([0.0, -1.0, 0.0]), c, np.array([1, 0, 0], dtype=F))
    assert tie[1] == 1.0 and tie[3] == -2.0


@pytest.mark.parametrize("name", sorted(SC.ground_cases()))
def test_ground_case_partitions_the_cloud(name):
    cloud, _ = SC.ground_cases()[name]
    g, o = SC.ground_answer(name)
    assert np.array_equal(np.sort(np.concatenate([g, o])), np.arange(cloud[0].size))
    assert (np.diff(g.astype(np.int64)) > 0).all() and (np.diff(o.astype(np.int64)) > 0).all()


def test_ground_cases_cover_what_the_table_promises():
    assert sorted({c[0][0].size for c in SC.ground_cases().values()}) == [1, 2, 255, 257, 300, 4097, 70000]
    # one point: a cell below min_points_per_cell is all obstacle; with min 1 / 0 the point is its own robust minimum
    assert SC.ground_answer("n1")[1].tolist() == [0]
    assert SC.ground_answer("n1_min1")[1].tolist() == [0]          # z = 3 is above max_ground_height
    assert SC.ground_answer("n1_min1_high")[0].tolist() == [0]
    assert SC.ground_answer("n1_min0")[1].tolist() == [0]
    assert SC.ground_answer("n2_zeros")[0].tolist() == [0, 1]      # -0.0 beside +0.0
    # negative coordinates, points exactly on cell edges
    x, y, _ = SC.ground_edges()
    assert (x < 0).any() and (y < 0).any() and (np.floor(x / F(0.5)) == x / F(0.5)).sum() >= 32
    # percentiles move the robust minimum (0: the cell's lowest z, 1: its highest), and 1.5 clamps to 1
    n_obst = {p: SC.ground_answer(k)[1].size for p, k in ((0, "n255_p0"), (1, "n255_p1"))}
    assert n_obst[0] != n_obst[1], n_obst
    assert np.array_equal(SC.ground_answer("n255_p1")[1], SC.ground_answer("n255_p1_5")[1])
    # the 0.3f grid: a division and a product with the reciprocal floor differently somewhere
    tx, ty, _ = SC.ground_thirds()
    assert SC.divide_and_multiply_differ(tx, 0.3).any() or SC.divide_and_multiply_differ(ty, 0.3).any()
    # z exactly at robust + thickness is ground, one ulp above is an obstacle; the high cell is all obstacle
    g, o = SC.ground_answer("n4097_exact_cut")
    assert {10, 11} <= set(g.tolist()) and {12, 13} <= set(o.tolist()) and set(range(10)) <= set(g.tolist())
    assert set(range(14, 24)) <= set(o.tolist())
    assert set(range(24, 30)) <= set(g.tolist())
    # the long cell and the one-point cells
    lx, ly, _ = SC.ground_large()
    cells = np.stack([np.floor(lx / F(0.5)), np.floor(ly / F(0.5))], axis=1)
    _, counts = np.unique(cells, axis=0, return_counts=True)
    assert counts.max() >= 5000 and (counts == 1).sum() >= 20000
    for name, (cloud, kw) in SC.ground_errors().items():
        with pytest.raises(ValueError):
            SR.segment_ground(*cloud, **kw)


# ---- the large cases, and the wide ones of the small table: admission and sensitivity ----
def coefficient_bits(r):
    return r["coefficients"].view(np.uint32).tolist()


@pytest.mark.parametrize("name", sorted(SL.plane_cases()))
def test_large_plane_case_is_admitted(name):
    base = SL.plane_answer(name)
    for order, solver in SL.ORDERS:  # (one loop, six refinements: the loop does not depend on either)
        r = SL.plane_answer(name, order, solver)
        assert coefficient_bits(r) == coefficient_bits(base), (order, solver)
        assert np.array_equal(r["inliers"], base["inliers"]), (order, solver)
    assert base["success"] and base["moments"] is not None and base["quotients"]
    for q in base["quotients"]:
        assert abs(q - round(q)) >= 1e-9, q
    n_list = SL.plane_loop(name)["indices"].size
    assert base["fitness"] == base["inliers"].size / float(n_list)


def test_plane_sum_cases_give_the_fixed_tree_a_second_term():
    counts = {}
    for name in SL.sum_cases():
        loop = SL.plane_loop(name)
        inl = SL.first_collect(name)  # what k_plane_sum sums over
        counts[name] = inl.size
        # sensitivity: the sums of the first 65 536 inliers alone (the stride skipped) refine to other coefficients
        full, _ = SR.refine(*loop["cloud"], inl, loop["best_model"])
        cut, _ = SR.refine(*loop["cloud"], inl[:SL.PLANE_SUM_SWEEP], loop["best_model"])
        assert full.view(np.uint32).tolist() != cut.view(np.uint32).tolist(), name
        assert coefficient_bits(SL.plane_answer(name)) == full.view(np.uint32).tolist()
        # the second collect is past the grid too (the engine refines once; both compactions cross 65 536)
        assert SL.plane_answer(name)["inliers"].size > SL.PLANE_SUM_SWEEP
    print(counts)
    assert SL.PLANE_SUM_SWEEP < counts["sum_one_block"] <= SL.PLANE_SUM_SWEEP + 256  # block 0 alone strides
    assert 95000 <= counts["sum_100k"] <= 105000


def test_plane_count_cases_make_a_second_sweep_that_decides():
    head = SL.count_loop("head")
    n_base = SL.count_base()[0].size
    assert head["indices"].size == SL.PLANE_COUNT_SWEEP and 200000 <= n_base <= 400000
    for name, (cloud, kw) in SL.count_cases().items():
        loop, r = SL.plane_loop(name), SL.plane_answer(name)
        m = loop["indices"].size
        assert m == SL.PLANE_COUNT_SWEEP + (1 if "_t1_" in name else SL.COUNT_TAIL)
        assert (cloud[0].size == m) == name.endswith("_cloud")
        if name.endswith("_list"):
            assert np.unique(kw["indices"]).size < kw["indices"].size <= 10 * n_base  # duplicates, a few per point
            assert np.array_equal(kw["indices"][:SL.PLANE_COUNT_SWEEP], head["indices"])
        # run to the cap: one batch of 128, the j >= 64 half of k_plane_count included
        assert r["iterations"] == loop["loop_iterations"] == kw["max_iterations"] == SC.BATCH
        # sensitivity, as the issue states it: the restatement over the first 2 097 152 entries alone differs
        assert (head["loop_iterations"], head["best_model"].view(np.uint32).tolist()) != \
               (loop["loop_iterations"], loop["best_model"].view(np.uint32).tolist()), name
    # ... and for the long tail with the loop's OWN 128 hypotheses, each scored against the first sweep alone (what
    # k_plane_count without its stride counts): another pass wins, with another model
    full, first_sweep = SL.first_sweep_winner("count_tail_list")
    assert full != first_sweep and full >= 0 and first_sweep >= 0
    # (the single entry of the T = 1 variant moves no count by more than one: it pins the lone live lane of block 0's
    # second tile — a count past m or a fault if its neighbours were not masked — not the winner)
    # plane B wins the whole list, plane A wins its first sweep
    loop = SL.plane_loop("count_tail_list")
    lx, ly, lz = (v[loop["indices"]] for v in loop["cloud"])
    cut = SL.PLANE_COUNT_SWEEP
    count = lambda model, upto: int(np.count_nonzero(SR.plane_dist(model, lx[:upto], ly[:upto], lz[:upto]) < loop["threshold"]))  # noqa: E731
    winner, other = loop["best_model"], head["best_model"]
    assert count(winner, None) == loop["best_count"] > count(other, None)
    assert count(winner, cut) < count(other, cut)
    # the cloud variant holds the list's points in the list's order: the two share their loop and their coefficients
    for t in ("count_t1", "count_tail"):
        a, b = SL.plane_answer(t + "_list"), SL.plane_answer(t + "_cloud")
        assert coefficient_bits(a) == coefficient_bits(b)
        assert np.array_equal(a["inliers"], SL.count_cases()[t + "_list"][1]["indices"][b["inliers"]])


def test_index_check_stride_list_is_bad_at_its_last_entry_only():
    cloud, _ = SC.INDEX_ERROR
    idx = SL.index_check_stride(cloud[0].size)
    assert idx.size == SL.INDEX_CHECK_SWEEP + 1 and int(idx[:-1].max()) < cloud[0].size == int(idx[-1])
    with pytest.raises(ValueError):
        SR.segment_plane(*cloud, distance_threshold=0.05, indices=idx, max_iterations=1)


@pytest.mark.parametrize("name", sorted(SL.ground_cases()))
def test_ground_600k_crosses_the_sort_tile_and_the_scan_carry(name):
    cloud, kw = SL.ground_cases()[name]
    n = cloud[0].size
    g, o = SL.ground_answer(name)
    assert np.array_equal(np.sort(np.concatenate([g, o])), np.arange(n))
    assert (np.diff(g.astype(np.int64)) > 0).all() and (np.diff(o.astype(np.int64)) > 0).all()
    assert n > SL.RS_SMALL_MAX  # rs_tile(n) = 4096 for both sorts
    cells = np.stack([np.floor(cloud[0] / F(0.5)), np.floor(cloud[1] / F(0.5))], axis=1)
    _, counts = np.unique(cells, axis=0, return_counts=True)
    assert (counts >= 5000).sum() >= 3 and ((counts == 1) | (counts == 2)).sum() > SL.SCAN_CHUNK
    assert counts.size > SL.SCAN_CHUNK  # the run heads' scan carries too
    # sensitivity: without the scan's carry the compaction of either list is another list
    for kept in (g, o):
        keep = np.zeros(n, dtype=bool)
        keep[kept] = True
        assert kept.size > 4096 and not np.array_equal(SL.compact_without_carry(keep), kept)
        assert np.array_equal(SL.compact_without_carry(keep[:SL.SCAN_CHUNK]), kept[kept < SL.SCAN_CHUNK])  # (the model)


@pytest.mark.parametrize("kind", sorted(SC.GROUND_WIDE))
def test_ground_wide_cases_need_more_than_32_key_bits(kind):
    for name in ("wide_" + kind, "wide_" + kind + "_min1"):
        cloud, kw = SC.ground_cases()[name]
        bits_x, bits_y, keys = SC.ground_key_bits(cloud)
        assert (bits_x, bits_y) == SC.GROUND_WIDE[kind] and bits_x + bits_y > 32
        # several points share a cell at these magnitudes: equal x, y, different z
        cells, counts = np.unique(np.array(keys, dtype=object), return_counts=True)
        assert (counts >= 6).sum() >= 20
        g, o = SC.ground_answer(name)
        assert g.size and o.size
        # sensitivity: sorted and compared by the low 32 bits of the key alone, the lists are others
        tg, to = SC.ground_with_32_bit_keys(cloud, **kw)
        assert not np.array_equal(tg, g) and not np.array_equal(to, o)
    if kind == "extremes":  # the accepted extremes themselves
        gx, gy = (SR.cell_coordinates(v, 0.5) for v in cloud[:2])
        assert gx.min() == gy.min() == -2.0 ** 31 and gx.max() == gy.max() == float(np.nextafter(F(2.0 ** 31), F(0)))
    if kind == "bits64":
        assert np.abs(cloud[0]).min() > 0.999e9 and (cloud[0] > 0).any() and (cloud[0] < 0).any()
    # the first refused floor is 2^31 itself
    bad = SC.ground_errors()["floor_exactly_2_31"][0][0]
    assert SR.cell_coordinates(bad, 0.5).max() == 2.0 ** 31


# ---- the engine's host algebra, stand-alone and sanitized ----
PROBE = os.path.join(ROOT, "fastdem_amd", "cpp", "tests", "seg_host_probe.cpp")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("seg_host") / "seg_host_probe")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "fastdem_amd", "csrc"), PROBE, "-o", exe])

    def run(*numbers):
        text = " ".join(float(v).hex() for v in numbers)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return [float.fromhex(tok) for tok in r.stdout.split()]
    return run


def test_host_sampler_draws_the_reference_triplets(probe):
    for n in (3, 4, 10, 500):
        got = np.array(probe(1, n, 1000), dtype=np.int64).reshape(1000, 3)
        want = np.array(SR.triplets(n, 1000), dtype=np.int64)
        assert np.array_equal(got, want), n
        assert (got[:, 0] != got[:, 1]).all() and (got[:, 2] != got[:, 0]).all() and (got[:, 2] != got[:, 1]).all()


def test_host_replay_stops_where_the_sequential_loop_stops(probe):
    for name, (cloud, kw) in SC.plane_cases().items():
        r = SC.plane_answer(name)
        idx = kw.get("indices")
        n_list = cloud[0].size if idx is None else idx.size
        if n_list < 3:
            continue
        passes = r["loop_iterations"]
        counts, valid = r["counts"], r["valid"]
        assert len(counts) == passes == len(valid)
        best = max([c for c, v in zip(counts, valid) if v], default=0)
        first = next((k for k, (c, v) in enumerate(zip(counts, valid)) if v and c == best), -1) if best else -1
        for batch in (1, 7, 64, 1000):
            got = probe(2, n_list, kw.get("max_iterations", 1000), kw.get("probability", 0.99), batch, passes, *counts, *valid)
            assert got == [float(passes), float(best), float(first), float(valid.count(0))], (name, batch, got)


def test_host_adaptive_iterations(probe):
    for ratio in (0.0, 1e-9, 0.12, 0.2, 0.3, 0.45, 0.5, 0.999999, 1.0, 1.5, -0.1):
        for p in (0.99, 0.5, 0.0, 1.0, 0.999999):
            assert probe(3, ratio, p) == [float(SR.adaptive_iterations(ratio, p))], (ratio, p)


def test_host_jacobi_agrees_with_eigh_to_the_float_cast(probe):
    seen = 0
    for name in SC.plane_cases():
        r = SC.plane_answer(name)
        if r["moments"] is None:
            continue
        seen += 1
        mom = r["moments"]
        cov = np.array([[mom[0], mom[1], mom[2]], [mom[1], mom[3], mom[4]], [mom[2], mom[4], mom[5]]])
        want = np.linalg.eigh(cov)[1][:, 0]
        got = np.array(probe(4, *mom))
        if got @ want < 0:
            got = -got
        assert np.array_equal(got.astype(F), want.astype(F)), (name, got, want)
        assert np.array_equal(np.array(probe(4, *mom)), SR.jacobi_smallest(mom)), name  # the same algorithm, bit for bit
        cloud, kw = SC.plane_cases()[name]
        c, _ = SR.moments(*cloud, SR.collect(*cloud, np.arange(cloud[0].size, dtype=np.uint32) if kw.get("indices") is None
                                             else kw["indices"], r["unrefined"], F(kw["distance_threshold"])))
        model = np.array(probe(5, *got, *c, *r["unrefined"][:3]), dtype=F)
        assert np.array_equal(model.view(np.uint32), SR.refined_model(got, c, r["unrefined"][:3]).view(np.uint32)), name
    assert seen >= 8
    # a diagonal matrix, a matrix with a zero off-diagonal pair, a rank-one matrix
    for mom in ([3.0, 0.0, 0.0, 2.0, 0.0, 1.0], [2.0, 1.0, 0.0, 2.0, 0.0, 0.5], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]):
        v = np.array(probe(4, *mom))
        cov = np.array([[mom[0], mom[1], mom[2]], [mom[1], mom[3], mom[4]], [mom[2], mom[4], mom[5]]])
        lam = np.linalg.eigvalsh(cov)[0]
        assert abs(np.linalg.norm(v) - 1.0) < 1e-12 and np.linalg.norm(cov @ v - lam * v) < 1e-12, mom
