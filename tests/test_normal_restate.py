"""tests/normal_restate.py against the known answers of the reference's own tests
(lib/nanoPCL/tests/test_geometry.cpp, its seventeen cases at its own tolerances; the cases that hand over a pre-built
tree run the plain function, the mirror having no KdTree), the properties the GPU tests rely on, and — for every cloud
of tests/normal_cases.py — the proof that it reaches the path of the search it is meant to reach.  CPU only."""
import numpy as np
import pytest

import dem_restate as DR
import normal_cases as NC
import normal_restate as NR

F32 = np.float32
CENTER = 12                                                          # (2, 2) of the 5 x 5 lattices


def est(cloud, k, viewpoint=(0.0, 0.0, 0.0)):
    return NR.estimate(*cloud, k, viewpoint)


def norm(v):
    return float(np.sqrt((v.astype(np.float64) ** 2).sum()))


# ---- Normal Estimation (test_geometry.cpp:82-188) ----
def test_normals_plane_xy():
    n = est(NC.plane_xy(5), 10)[0][CENTER]
    assert abs(abs(n[0]) - 0) < 0.1 and abs(abs(n[1]) - 0) < 0.1 and abs(abs(n[2]) - 1) < 0.1


def test_normals_plane_xz():
    n = est(NC.plane_xz(5), 10)[0][CENTER]
    assert abs(abs(n[0]) - 0) < 0.1 and abs(abs(n[1]) - 1) < 0.1 and abs(abs(n[2]) - 0) < 0.1


def test_normals_plane_arbitrary():
    n = est(NC.plane_tilted(5), 10)[0][CENTER]
    e = np.array([-0.5, -0.3, 1.0], dtype=F32)
    e = e / F32(np.sqrt((e * e).sum()))
    assert abs(abs(float((n * e).sum())) - 1.0) < 0.1


def test_normals_viewpoint_orientation():
    cloud = NC.plane_xy(5)
    vp = np.array([2.0, 2.0, 10.0], dtype=F32)
    n = est(cloud, 10, tuple(vp))[0][CENTER]
    to_vp = vp - np.array([c[CENTER] for c in cloud], dtype=F32)
    assert float((n * to_vp).sum()) > 0


def test_normals_viewpoint_below():
    assert est(NC.plane_xy(5), 10, (2.0, 2.0, -10.0))[0][CENTER][2] < 0


def test_normals_sparse_cloud():
    n = est(NC.sparse(), 10)[0]
    assert norm(n[0]) < 1e-5 and norm(n[1]) < 1e-5


def test_normals_with_external_kdtree():
    assert abs(abs(est(NC.plane_xy(5), 10)[0][CENTER][2]) - 1.0) < 0.1


# ---- Covariance Estimation (:194-260) ----
def test_covariances_planar():
    w = np.linalg.eigvalsh(est(NC.plane_xy(5), 10)[1][CENTER].astype(np.float64))
    assert abs(w[0] - 1e-3) < 1e-4 and abs(w[1] - 1.0) < 0.1 and abs(w[2] - 1.0) < 0.1


def test_covariances_gicp_regularization():
    c = est(NC.plane_xy(5), 10)[1][CENTER]
    assert abs(c[0, 1] - c[1, 0]) < 1e-6 and abs(c[0, 2] - c[2, 0]) < 1e-6 and abs(c[1, 2] - c[2, 1]) < 1e-6
    assert (np.linalg.eigvalsh(c.astype(np.float64)) >= 0).all()


def test_covariances_invalid_returns_identity():
    c = est(NC.sparse(), 10)[1][0]
    assert abs(c[0, 0] - 1) < 1e-5 and abs(c[1, 1] - 1) < 1e-5 and abs(c[2, 2] - 1) < 1e-5 and abs(c[0, 1]) < 1e-5


def test_covariances_with_external_kdtree():
    assert np.trace(est(NC.plane_xy(5), 10)[1][CENTER]) > 0


# ---- Combined (:266-305) ----
def test_normals_covariances_single_pass():
    """The restatement computes the pair from one PCA, as NormalCovarianceSetter does; the two separate functions run the
    same search and the same PCA, so the reference's 1e-5 is met with 0: bit for bit."""
    cloud = NC.plane_xy(5)
    n1, c1, _ = est(cloud, 10)
    n2 = NR.estimate(*cloud, 10, setter="normal")[0]                 # estimateNormals
    c2 = NR.estimate(*cloud, 10, setter="covariance")[1]             # estimateCovariances
    assert np.array_equal(n1.view(np.uint32), n2.view(np.uint32)) and np.array_equal(c1.view(np.uint32), c2.view(np.uint32))
    for i in range(25):
        assert norm(n1[i] - n2[i]) < 1e-5 and norm((c1[i] - c2[i]).reshape(-1)) < 1e-5


def test_normals_covariances_with_external_kdtree():
    n, c, bad = est(NC.plane_xy(5), 10)
    assert n.shape == (25, 3) and c.shape == (25, 3, 3) and not bad.any()


# ---- Edge Cases (:311-357) ----
def test_empty_cloud():
    e = np.zeros(0, dtype=F32)
    n, c, bad = NR.estimate(e, e, e, 10)
    assert n.shape == (0, 3) and c.shape == (0, 3, 3) and bad.size == 0


def test_single_point():
    n, _, bad = NR.estimate(np.array([1], dtype=F32), np.array([2], dtype=F32), np.array([3], dtype=F32), 10)
    assert norm(n[0]) < 1e-5 and bad.all()


def test_collinear_points():
    n, c, _ = est(NC.collinear(), 5)                                 # "just verify no crash and channel is set"
    assert n.shape == (10, 3) and np.isfinite(n).all() and np.isfinite(c).all()


def test_normal_unit_length():
    for v in est(NC.plane_xy(5), 10)[0]:
        assert norm(v) < 1e-5 or abs(norm(v) - 1.0) < 1e-5


# ---- properties ----
@pytest.mark.parametrize("name,k", [("surface", 20), ("utm", 20), ("tilted10", 10), ("duplicates", 10)])
def test_valid_normals_have_unit_length(name, k):
    _, _, n, _, bad = NC.restated(name, k)
    length = np.sqrt((n[~bad].astype(np.float64) ** 2).sum(axis=1))
    assert (~bad).any() and np.abs(length - 1.0).max() < 1e-5
    assert not n[bad].any()


@pytest.mark.parametrize("name", ["xy5", "xy10", "xz10", "tilted10"])
def test_planar_covariance_has_the_gicp_eigenvalues(name):
    _, _, _, c, bad = NC.restated(name, 10)
    assert not bad.any()
    w = np.linalg.eigvalsh(c.astype(np.float64))
    assert np.abs(w - np.array([1e-3, 1.0, 1.0])).max() < 1e-5


def test_lattices_meet_the_references_expectations():
    """The ties of the integer lattices are broken by index here and by the tree's traversal in the reference; what the
    reference's tests ask of them holds whichever way."""
    for name, axis in (("xy5", 2), ("xy10", 2), ("xz5", 1), ("xz10", 1)):
        n = NC.restated(name, 10)[2]
        assert (np.abs(np.abs(n[:, axis]) - 1.0) < 0.1).all() and (np.abs(np.delete(n, axis, axis=1)) < 0.1).all(), name
    e = np.array([-0.5, -0.3, 1.0]) / np.sqrt(0.25 + 0.09 + 1.0)
    for name in ("tilted5", "tilted10"):
        n = NC.restated(name, 10)[2].astype(np.float64)
        assert (np.abs(np.abs(n @ e) - 1.0) < 0.1).all(), name


def test_a_dot_of_exactly_zero_does_not_flip():
    cloud = NC.plane_xy(5)
    raw = NR.estimate(*cloud, 10, None)[0]                           # column 0 as the solver leaves it
    got = NC.restated("xy5", 10, (2.0, 2.0, 0.0))[2]                 # the viewpoint in the plane
    P = np.stack(cloud, axis=1)
    assert (NR.dot3(raw, np.array([2, 2, 0], dtype=F32)[None, :] - P) == 0).all()
    assert np.array_equal(got.view(np.uint32), raw.view(np.uint32))
    above, below = NC.restated("xy5", 10, (2.0, 2.0, 10.0))[2], NC.restated("xy5", 10, (2.0, 2.0, -10.0))[2]
    assert (above[:, 2] > 0).all() and (below[:, 2] < 0).all()
    assert np.array_equal(above.view(np.uint32), (-below).view(np.uint32))


def test_a_smaller_k_is_a_prefix_of_the_neighbour_table():
    x, y, z = NC.cloud("duplicates")
    rows = np.arange(x.size)
    assert np.array_equal(NR.neighbours(x, y, z, 10, rows), NR.neighbours(x, y, z, 64, rows)[:, :10])


# ---- which path each case cloud reaches ----
def test_isolated_points_lie_beyond_four_rings():
    """NC.must_queue states the argument.  All six far points up to k = 33; at k = 64 the columns are 16 m wide and four
    and a half of them reach the patch from three of the six."""
    x, y, _ = NC.cloud("isolated")
    assert np.flatnonzero(np.maximum(np.abs(x), np.abs(y)) > 30).size == 6
    counts = {k: NC.must_queue("isolated", k) for k in (3, 4, 5, 16, 17, 20, 32, 33, 64)}
    assert all(c >= 1 for c in counts.values()), counts
    assert all(counts[k] == 6 for k in (3, 4, 5, 16, 17, 20, 32, 33)) and counts[64] == 3, counts


def test_small_grid_is_covered_by_four_rings_from_anywhere():
    for k in (10, 20):
        _, gx, gy, _, _ = NC.grid_of("small_grid", k)
        assert 1 < gx <= NC.SHELLS + 1 and 1 < gy <= NC.SHELLS + 1


def test_degenerate_clouds_are_what_they_claim():
    x, y, z = NC.cloud("identical")
    assert DR.sor_grid(x.min(), y.min(), x.max(), y.max(), x.size, 10)[1:] == (1, 1)   # a box without area: one column
    _, _, n, c, bad = NC.restated("identical", 10)
    assert bad.all() and not n.any() and np.array_equal(c, np.tile(np.eye(3, dtype=F32), (100, 1, 1)))
    assert not NC.restated("collinear", 5)[4].any()                  # a line is not degenerate to the trace test
    x, y, z = NC.cloud("duplicates")
    idx = NR.neighbours(x, y, z, 10, np.array([150]))[0]
    assert list(idx[:5]) == [3, 77, 150, 151, 290]                   # the copies first, by index: lower and higher than 150


def test_the_utm_offset_matters():
    """At 5e5 an fp32 step is 1/32 m: the sums are only usable because they are taken relative to the first neighbour."""
    (x, y, z), _, n, _, bad = NC.restated("utm", 20)
    assert not bad.any() and float(np.spacing(F32(5.0e5))) == 0.03125
    P = np.stack([x, y, z], axis=1).astype(np.float64)
    idx = NC._table("utm")[:, :20]
    plain = np.array([np.cov((P[i] - P[i].mean(axis=0)).T, bias=True) for i in idx[:64]])
    w, v = np.linalg.eigh(plain)
    assert (np.abs((v[:, :, 0] * n[:64].astype(np.float64)).sum(axis=1)) > 0.999).all()


def test_bucket_edges_and_sizes_are_covered():
    assert [DR.MAX_K, NR.MAX_K] == [64, 64]
    for k, n in ((3, 4096), (64, 4096), (-1, 10), (10, 5), (-1, 3)):
        assert NR.MIN_NEIGHBORS <= NR.effective_k(n, k) <= NR.MAX_K
    assert NR.effective_k(257, -1) == 257 and NR.effective_k(2, 10) == 2 and NR.effective_k(0, 10) == 0
