"""Cloud registration on the device (fastdem_amd/csrc/fdm_register.hpp, fdm_cloud_register and
fdm_cloud_register_linearize) against the NumPy restatement of nanoPCL's alignICP / alignPlaneICP / alignGICP
(tests/reg_restate.py).  One linearization is held tightly: the same inliers, and every one of the 28 sums within
(2 n + 32) 2^-53 sum|term| of the correctly rounded sum for ICP and plane ICP — two summations of n doubles and a few
roundings per term — and within 1e-9 sum|term| for GICP, where the two sides' eigen-solvers differ by about 1e-14 in
C_reg at an eigen-gap of 0.9 and cond(C_src + C_tgt) <= 1e3.  align is held on the cases tests/test_reg_restate.py
admits: the same iterations, converged and fitness, the transform and rmse within 64 x the case's recorded spread between
summation orders (floor 1e-13).

Run on the GPU box:  python -m pytest tests -m gpu
"""
import ctypes as C
import math

import numpy as np
import pytest

import reg_cases as RC
import reg_restate as RR

pytestmark = pytest.mark.gpu
F32 = np.float32
KERNEL_NAMES = {RR.NONE: "none", RR.HUBER: "huber", RR.TUKEY: "tukey", RR.CAUCHY: "cauchy"}


def settings_of(problem):
    return dict(problem.set)


def to_device(v):
    import torch
    return None if v is None else torch.from_numpy(np.array(v, dtype=F32)).cuda()   # (copies: the cases are read-only)


def inputs(problem, on_device=False):
    s, t, raw = list(problem.s), list(problem.t), dict(problem.raw)
    if on_device:
        s, t = [to_device(v) for v in s], [to_device(v) for v in t]
        raw = {k: to_device(v) for k, v in raw.items()}
    return s, t, raw


def linearize(gpu, problem, T, on_device=False):
    s, t, raw = inputs(problem, on_device)
    out = gpu.linearize(problem.method, *s, *t, transform=T, return_correspondences=True, **raw, **settings_of(problem))
    if on_device:
        out["corr"] = out["corr"].cpu().numpy()
    return out


def align(gpu, problem, guess=None, on_device=False):
    s, t, raw = inputs(problem, on_device)
    fn = {"icp": gpu.align_icp, "plane": gpu.align_plane_icp, "gicp": gpu.align_gicp}[problem.method]
    extra = {"icp": (), "plane": (raw["target_normals"],), "gicp": (raw["source_cov"], raw["target_cov"])}[problem.method]
    return fn(*s, *t, *extra, initial_guess=guess, **settings_of(problem))


def check_linearize(gpu, problem, T, label):
    want = problem.linearize(T)
    got = linearize(gpu, problem, T)
    assert got["num_inliers"] == want["num_inliers"], label
    assert np.array_equal(got["corr"].astype(np.int64), want["corr"]), label
    sums = np.concatenate([got["H_upper"], got["b"], [got["error"]]])
    diff = np.abs(sums - want["sums"])
    if problem.method == "gicp":
        limit = 1e-9 * want["abs_sums"]
    else:
        limit = RC.bound(problem.n, want["abs_sums"])
    worst = float(np.max(np.where(limit > 0, diff / np.where(limit > 0, limit, 1.0), np.where(diff > 0, np.inf, 0.0))))
    print(f"{label}: {want['num_inliers']}/{problem.n} inliers, worst sum at {worst:.3g} of its bound")
    assert (diff <= limit).all(), (label, np.flatnonzero(diff > limit), diff, limit)
    assert np.array_equal(got["H"], got["H"].T)
    return want, got


# ---- 1. linearize against the restatement ----
COMBOS = [("icp", RR.NONE)] + [(m, k) for m in ("plane", "gicp") for k in (RR.NONE, RR.HUBER, RR.TUKEY, RR.CAUCHY)]


@pytest.mark.parametrize("method,kernel", COMBOS, ids=[f"{m}-{KERNEL_NAMES[k]}" for m, k in COMBOS])
def test_linearize_against_the_restatement(gpu, method, kernel):
    proper = 0
    for ns, nt in RC.lin_shapes():
        problem = RC.lin_problem(method, kernel, ns, nt)
        for ti, T in enumerate(RC.lin_transforms()):
            want, _ = check_linearize(gpu, problem, T, f"{method} {KERNEL_NAMES[kernel]} {ns} x {nt} T{ti}")
            proper += 0 < want["num_inliers"] < ns
    assert proper >= 10                                              # the inliers were a proper subset: the mask matters


def test_the_robust_kernels_change_the_sums(gpu):
    """The kernel argument reaches the factor: at these widths every kernel gives another error sum."""
    for method in ("plane", "gicp"):
        errors = [linearize(gpu, RC.lin_problem(method, k, 1000, 1000), np.eye(4))["error"] for k in range(4)]
        assert len(set(errors)) == 4, (method, errors)
    icp = [linearize(gpu, RC.lin_problem("icp", k, 1000, 1000), np.eye(4))["error"] for k in range(4)]
    assert len(set(icp)) == 1                                        # ICP has none


# ---- 2. search edges ----
def cloud_of(points):
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    return tuple(np.ascontiguousarray(p[:, a]) for a in range(3))


def check_search(gpu, source, target, max_dist, T=None, label=""):
    problem = RR.Problem("icp", source, target, max_correspondence_dist=max_dist)
    want, got = check_linearize(gpu, problem, np.eye(4) if T is None else T, label)
    st = gpu.register_last_stats()
    assert st["ring_limit"] == RC.ring_limit(st["grid_x"], st["grid_y"], st["voxel"], max_dist), st
    assert st["n_source"] == source[0].size and st["n_target"] == target[0].size and st["linearizations"] == 1
    assert st["ms"] == (0.0, 0.0, 0.0)                               # no events unless fdm_cloud_debug_profile is on
    print(f"{label}: grid {st['grid_x']} x {st['grid_y']} of {st['voxel']:.4g}, ring limit {st['ring_limit']}")
    return want["corr"], st


def test_equidistant_targets_take_the_lower_index_in_both_orders(gpu):
    src = cloud_of([[0, 0, 0], [0, 0.5, 0]])
    corr, _ = check_search(gpu, src, cloud_of([[1, 0, 0], [-1, 0, 0], [5, 5, 0]]), 2.0, label="tie a")
    assert corr.tolist() == [0, 0]
    corr, _ = check_search(gpu, src, cloud_of([[5, 5, 0], [-1, 0, 0], [1, 0, 0]]), 2.0, label="tie b")
    assert corr.tolist() == [1, 1]
    corr, _ = check_search(gpu, src, cloud_of([[1, 0, 0]] * 3 + [[-1, 0, 0]] * 3), 2.0, label="tie of duplicates")
    assert corr.tolist() == [0, 0]


def test_the_radius_is_inclusive_to_the_ulp(gpu):
    above = float(np.nextafter(F32(0.5), F32(1.0)))
    src = cloud_of([[0.5, 0, 0], [above, 0, 0], [0, -0.5, 0], [0, 0, above]])
    tgt = cloud_of([[0, 0, 0], [9, 9, 9]])
    corr, _ = check_search(gpu, src, tgt, 0.5, label="radius")         # d2 = 0.25 = max_dist_sq: accepted; one ulp above: not
    assert corr.tolist() == [0, -1, 0, -1]


def test_queries_outside_the_targets_box_and_beyond_the_radius(gpu):
    tgt = RC.sphere(257)
    far = [[s * d if a == k else 0.0 for a in range(3)] for d in (1.05, 1.2, 3.0, 50.0) for k in range(3) for s in (1, -1)]
    corr, st = check_search(gpu, cloud_of(far + [[0.9, 0.9, 0.0], [-2.0, -2.0, 0.0]]), tgt, 0.3, label="outside")
    assert (corr >= 0).any() and (corr < 0).any()
    assert st["ring_limit"] < max(st["grid_x"], st["grid_y"]) - 1      # ended by the radius exit, not by the grid


def test_degenerate_targets(gpu):
    src = cloud_of([[1, 2, 3], [1.1, 2, 3], [4, 2, 3], [1, 2, 3.2]])
    corr, st = check_search(gpu, src, cloud_of([[1, 2, 3]] * 50), 0.25, label="identical")
    assert (st["grid_x"], st["grid_y"], st["ring_limit"]) == (1, 1, 0) and corr.tolist() == [0, 0, -1, 0]
    line = cloud_of([[0.1 * i, 7.0, 0.0] for i in range(100)])
    src = cloud_of([[0.52, 7.0, 0.0], [0.52, 7.3, 0.0], [-0.3, 7.0, 0.0], [10.2, 7.0, 0.1], [5.0, 8.0, 0.0], [5.04, 7.0, 0.0]])
    corr, st = check_search(gpu, src, line, 0.4, label="line")
    assert st["grid_y"] == 1 and st["grid_x"] > 1
    assert corr.tolist() == [5, 5, 0, 99, -1, 50]


def test_whole_grid_exit_and_a_radius_larger_than_the_grid(gpu):
    g = np.random.default_rng(3)
    small = cloud_of(np.concatenate([g.uniform(0, 1, (30, 2)), np.zeros((30, 1))], axis=1))
    src = cloud_of([[5, 5, 0], [-3, 0.5, 0], [0.5, 0.5, 2.0], [0.5, 0.5, 0.0]])
    corr, st = check_search(gpu, src, small, 10.0, label="whole grid")
    assert st["ring_limit"] == max(st["grid_x"], st["grid_y"]) - 1 and (corr >= 0).all()
    problem = RC.lin_problem("icp", RR.NONE, 257, 1000)
    corr, st = check_search(gpu, problem.s, problem.t, 100.0, RC.lin_transforms()[2], label="radius beyond the grid")
    assert st["ring_limit"] == max(st["grid_x"], st["grid_y"]) - 1 and (corr >= 0).all()


def test_utm_sized_offsets(gpu):
    off = np.array([5.0e5, 4.9e5, 150.0])
    shift = lambda c: tuple((v.astype(np.float64) * 20.0 + o).astype(F32) for v, o in zip(c, off))   # noqa: E731
    src, tgt = shift(RC.sphere(769, 43)), shift(RC.sphere(1000, 42))
    T = RR.se3_exp([0.3, -0.2, 0.1, 0.0, 0.0, 1e-6])
    for k, t in enumerate((np.eye(4), T)):
        corr, _ = check_search(gpu, src, tgt, 2.0, t, label=f"utm T{k}")
        assert 0 < (corr >= 0).sum() < 769


# ---- 3. align against the restatement ----
@pytest.mark.parametrize("name", RC.ALIGN_CASES)
def test_align_against_the_restatement(gpu, name):
    case = RC.align_case(name)
    want = case.restated("forward")
    got = align(gpu, case.problem, case.guess)
    tol = max(64.0 * case.spread, 1e-13)
    dT = float(np.linalg.norm(got.transform - want.transform))
    print(f"{name}: iterations {got.iterations}, converged {got.converged}, fitness {got.fitness:.4f}, rmse {got.rmse:.6e}, "
          f"|dT| {dT:.3e} (tolerance {tol:.1e}), |d rmse| {abs(got.rmse - want.rmse) if math.isfinite(want.rmse) else 0.0:.3e}")
    assert (got.iterations, got.converged) == (want.iterations, want.converged)
    assert got.fitness == want.fitness
    assert dT <= tol
    if math.isinf(want.rmse):
        assert math.isinf(got.rmse) and got.rmse > 0
    else:
        assert abs(got.rmse - want.rmse) <= tol
    st = gpu.register_last_stats()
    assert st["linearizations"] == (want.iterations if want.converged or name.startswith("icp_max") or name == "partial_overlap"
                                    else want.iterations + 1)
    if case.tol is not None:
        assert RR.transform_error(got.transform, case.gt) < case.tol
    if name in RC.SPHERE_CASES:
        inv = np.linalg.inv(want.H)
        assert got.covariance is not None
        assert np.abs(got.covariance - inv).max() <= 64.0 * np.linalg.cond(want.H) * 2.0 ** -53 * np.abs(inv).max()
    if name == "perfect_plane":
        assert got.covariance is None and want.covariance is None
    if name == "sparse":
        assert got.covariance is None and np.array_equal(got.transform, np.eye(4))


def test_min_correspondences_nine_fail_and_ten_pass(gpu):
    pts = np.stack(RC.sphere(12), axis=1).astype(np.float64) * 3.0    # twelve points well apart, not in a plane
    tgt = cloud_of(pts)
    near = (pts[:10] + [0.01, 0.02, 0.0]).tolist()
    for inliers, ok in ((9, False), (10, True)):
        src = cloud_of(near[:inliers] + [[i, 50, 0] for i in range(12 - inliers)])
        # (one iteration: the check is the first thing it does, and what ICP makes of ten points is not the subject)
        problem = RR.Problem("icp", src, tgt, max_correspondence_dist=0.5, min_correspondences=10, max_iterations=1)
        want, got = RR.align(problem), align(gpu, problem)
        assert want.num_inliers == inliers and want.iterations == int(ok) and want.fitness == (10 / 12 if ok else 0.0)
        assert (got.iterations, got.converged, got.fitness) == (want.iterations, want.converged, want.fitness)
        if not ok:
            assert got.iterations == 0 and not got.converged and got.fitness == 0.0 and math.isinf(got.rmse)
            assert got.covariance is None and np.array_equal(got.transform, np.eye(4))


def test_no_iterations_returns_the_initial_guess(gpu):
    c = RC.sphere(257)
    guess = RC.random_transform(0.3, 0.15, 9)
    got = align(gpu, RR.Problem("icp", c, c, max_iterations=0), guess)
    assert got.iterations == 0 and not got.converged and got.fitness == 0.0 and math.isinf(got.rmse)
    assert got.covariance is None and np.array_equal(got.transform, guess)
    assert gpu.register_last_stats()["linearizations"] == 0


def test_no_inliers_allowed_converges_with_a_nan_rmse_as_in_the_reference(gpu):
    """min_correspondences = 0 and nothing in reach: H = 0, b = 0, delta = 0, converged — and makeSuccessResult divides
    0 by 0 inliers without a guard."""
    far = RC.transform_cloud(RC.sphere(63), RC.translation(50.0, 0.0, 0.0))
    problem = RR.Problem("icp", far, RC.sphere(257), min_correspondences=0)
    want, got = RR.align(problem), align(gpu, problem)
    assert want.converged and want.iterations == 1 and math.isnan(want.rmse)
    assert got.converged and got.iterations == 1 and got.fitness == 0.0 and math.isnan(got.rmse) and got.covariance is None
    assert np.array_equal(got.transform, np.eye(4))


def test_identical_clouds_stall_at_once(gpu):
    got = align(gpu, RC.align_case("icp_identity").problem)
    assert got.converged and got.iterations == 1 and got.fitness == 1.0 and got.rmse == 0.0


def test_the_eps_names_are_swapped_as_in_the_reference(gpu):
    """translation_eps bounds |omega| and rotation_eps bounds |v| (criteria.hpp as written).  With relative_error_eps 0,
    translation_eps 4e-3 and rotation_eps 1 the reference's reading converges at the third iteration of this case, where
    |omega| falls to 1.7e-3 (5.1e-3 the iteration before) while |v| is still 3.7e-2; the other reading would need |v| below
    4e-3 and go on to the ninth."""
    base = RC.align_case("icp_rotation_translation").problem
    problem = RR.Problem("icp", base.s, base.t, max_iterations=100, relative_error_eps=0.0, translation_eps=4e-3,
                         rotation_eps=1.0)
    trace = []
    want = RR.align(problem, trace=trace)
    v, w = [np.linalg.norm(d[:3]) for d in trace], [np.linalg.norm(d[3:]) for d in trace]
    assert want.converged and want.iterations == 3
    assert w[2] < 4e-3 / 1.5 and w[1] > 4e-3 * 1.2 and v[2] > 4e-3 * 5        # away from the boundary, and v would not do
    got = align(gpu, problem)
    assert (got.iterations, got.converged) == (3, True)
    swapped = RR.Problem("icp", base.s, base.t, max_iterations=5, relative_error_eps=0.0, translation_eps=1.0,
                         rotation_eps=4e-3)
    got = align(gpu, swapped)
    assert (got.iterations, got.converged) == (5, False)             # |v| stays above 4e-3 through five iterations


# ---- 4. plumbing ----
def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("method", ["icp", "plane", "gicp"])
def test_host_and_device_arrays_and_repeated_calls_give_the_same_bits(gpu, method):
    problem = RC.lin_problem(method, RR.HUBER, 769, 1000)
    T = RC.lin_transforms()[1]
    a, b, c = linearize(gpu, problem, T), linearize(gpu, problem, T), linearize(gpu, problem, T, on_device=True)
    for other in (b, c):
        assert same_bits(a["H_upper"], other["H_upper"]) and same_bits(a["b"], other["b"])
        assert same_bits(a["error"], other["error"]) and np.array_equal(a["corr"], other["corr"])
    case = RC.align_case({"icp": "icp_translation", "plane": "plane_icp", "gicp": "gicp"}[method])
    r = [align(gpu, case.problem), align(gpu, case.problem), align(gpu, case.problem, on_device=True)]
    for other in r[1:]:
        assert same_bits(r[0].transform, other.transform) and same_bits(r[0].rmse, other.rmse)
        assert (r[0].iterations, r[0].fitness) == (other.iterations, other.fitness)
        assert same_bits(r[0].covariance, other.covariance)


def test_empty_clouds(gpu):
    e = tuple(np.zeros(0, dtype=F32) for _ in range(3))
    c = RC.sphere(63)
    guess = RC.random_transform(0.3, 0.15, 9)
    for s, t in ((e, c), (c, e), (e, e)):
        got = gpu.align_icp(*s, *t, initial_guess=guess)
        assert got.iterations == 0 and not got.converged and got.fitness == 0.0 and math.isinf(got.rmse)
        assert got.covariance is None and np.array_equal(got.transform, guess)
        lin = gpu.linearize("icp", *s, *t, return_correspondences=True)
        assert lin["num_inliers"] == 0 and not lin["H"].any() and lin["error"] == 0.0 and (lin["corr"] == -1).all()
    # the reference returns before it looks for the channels
    assert gpu.align_plane_icp(*e, *c, None).iterations == 0 and gpu.align_gicp(*c, *e, None, None).iterations == 0


def test_refusals_return_invalid_and_restore_the_device(gpu):
    """Every refusal of include/fdm_engine.h, by both entries.  The device: where a second one exists the thread is put on
    it and the calls run on device 0, so a call that did not put the thread's device back would leave it on 0; on a
    machine with one device the assertion cannot fail and proves nothing."""
    import torch
    other = torch.cuda.device_count() - 1                            # 0 where there is one device
    torch.cuda.set_device(other)
    lib, INVALID = gpu.capi.load(), gpu.capi.FDM_ERR_INVALID
    s, t, sc, tn, tc = RC.lin_base()
    keep = [np.ascontiguousarray(v) for v in (*s, *t)] + [np.ascontiguousarray(tn[:, a]) for a in range(3)] + \
        [np.ascontiguousarray(sc.transpose(0, 2, 1)), np.ascontiguousarray(tc.transpose(0, 2, 1))]
    P = [v.ctypes.data_as(C.c_void_p) for v in keep]
    res = gpu.capi.FdmRegistrationResult()

    def call(method=0, sx=P[0], tx=P[3], normals=(P[6], P[7], P[8]), scov=P[9], tcov=P[10], guess=None, **settings):
        clouds = gpu.capi.FdmRegisterClouds(1000, sx, P[1], P[2], scov, 1000, tx, P[4], P[5], *normals, tcov, 0)
        st = gpu.align_settings(**settings)
        g = None if guess is None else (C.c_double * 16)(*guess)
        before = torch.cuda.current_device()
        rc = lib.fdm_cloud_register(method, C.byref(clouds), g, C.byref(st), 0, C.byref(res))
        H, b, e, k = (C.c_double * 21)(), (C.c_double * 6)(), C.c_double(), C.c_uint64()
        rc2 = lib.fdm_cloud_register_linearize(method, C.byref(clouds), g, C.byref(st), 0, H, b, C.byref(e), C.byref(k), None)
        assert torch.cuda.current_device() == before == other and rc == rc2
        return rc

    assert call(0) == 0 and call(1) == 0 and call(2) == 0
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 3):                                         # a source, a target coordinate
            dirty = keep[which].copy()
            dirty[500] = bad
            p = dirty.ctypes.data_as(C.c_void_p)
            assert call(0, **({"sx": p} if which == 0 else {"tx": p})) == INVALID
        g = np.eye(4).reshape(16).copy()
        g[13] = bad
        assert call(0, guess=g) == INVALID
    assert call(1, normals=(P[6], None, P[8])) == INVALID and call(1, normals=(None, None, None)) == INVALID
    assert call(2, scov=None) == INVALID and call(2, tcov=None) == INVALID
    assert call(0, normals=(None, None, None), scov=None, tcov=None) == 0      # ICP needs neither
    assert call(0, max_correspondence_dist=-1.0) == INVALID and call(0, max_correspondence_dist=math.nan) == INVALID
    assert call(0, max_correspondence_dist=0.0) == 0
    assert call(3) == INVALID and call(-1) == INVALID and call(0, robust_kernel=4) == INVALID
    for ns, nt in ((1 << 31, 1000), (1000, 1 << 31)):                # more than the grid takes, in either cloud, by either entry
        clouds = gpu.capi.FdmRegisterClouds(ns, P[0], P[1], P[2], None, nt, P[3], P[4], P[5], None, None, None, None, 0)
        assert lib.fdm_cloud_register(0, C.byref(clouds), None, None, 0, C.byref(res)) == INVALID
        H, b, e, k = (C.c_double * 21)(), (C.c_double * 6)(), C.c_double(), C.c_uint64()
        assert lib.fdm_cloud_register_linearize(0, C.byref(clouds), None, None, 0, H, b, C.byref(e), C.byref(k), None) == INVALID
    with pytest.raises(gpu.EngineError):
        gpu.align_plane_icp(*s, *t, None)
    torch.cuda.set_device(0)
    with pytest.raises(TypeError):                                   # torch and NumPy mixed, a float64 tensor
        gpu.align_icp(*[to_device(v) for v in s], *t)
    with pytest.raises(TypeError):
        gpu.align_icp(*[to_device(v).double() for v in s], *[to_device(v) for v in t])


# The refusal texts, as fdm_last_error() gives them (the literals of fastdem_amd/csrc: fdm_engine_register.inl,
# fdm_engine_cloud.inl's check_cloud, fdm_engine_dem.inl's knn_grid_build).
MSG = {
    "null": "null argument",
    "method": "method must be 0 (ICP), 1 (PLANE) or 2 (GICP)",
    "kernel": "robust_kernel must be 0 (NONE), 1 (HUBER), 2 (TUKEY) or 3 (CAUCHY)",
    "max_dist": "max_correspondence_dist must not be negative or NaN",
    "transform": "the transform has an entry that is not finite",
    "count": "point count exceeds 2^31-1",
    "array": "null coordinate array",
    "normals": "alignPlaneICP: target must have normals (all of nx, ny, nz)",
    "source_cov": "alignGICP: source must have covariances",
    "target_cov": "alignGICP: target must have covariances",
    "source_finite": "the source cloud has a coordinate that is not finite",
    "target_finite": "the cloud has a coordinate that is not finite (undefined in the reference's k-d tree)",
}


CLEAN = object()                                                     # an argument left as lin_base() has it


class RawEntries:
    """fdm_cloud_register and fdm_cloud_register_linearize through ctypes on lin_base()'s clouds as host arrays; a call
    returns (return code, fdm_last_error()) after asserting that both entries agree on both."""

    def __init__(self, gpu):
        s, t, sc, tn, tc = RC.lin_base()
        self.gpu, self.lib = gpu, gpu.capi.load()
        self.keep = [np.ascontiguousarray(v) for v in (*s, *t)] + [np.ascontiguousarray(tn[:, a]) for a in range(3)] + \
            [np.ascontiguousarray(sc.transpose(0, 2, 1)), np.ascontiguousarray(tc.transpose(0, 2, 1))]
        self.P = [v.ctypes.data_as(C.c_void_p) for v in self.keep]

    def dirty(self, which, value=np.nan):
        """The pointer of a copy of array `which` with one entry replaced."""
        bad = self.keep[which].copy()
        bad[500] = value
        self.keep.append(bad)
        return bad.ctypes.data_as(C.c_void_p)

    def outputs(self):
        return [C.byref(self.gpu.capi.FdmRegistrationResult())], \
            [(C.c_double * 21)(), (C.c_double * 6)(), C.byref(C.c_double()), C.byref(C.c_uint64())]

    def __call__(self, method=0, ns=1000, nt=1000, sx=CLEAN, tx=CLEAN, normals=CLEAN, scov=CLEAN, tcov=CLEAN, guess=None,
                 clouds=CLEAN, null_output=None, **settings):
        P = self.P
        pick = lambda given, default: default if given is CLEAN else given   # noqa: E731
        if clouds is CLEAN:
            clouds = C.byref(self.gpu.capi.FdmRegisterClouds(ns, pick(sx, P[0]), P[1], P[2], pick(scov, P[9]), nt,
                                                             pick(tx, P[3]), P[4], P[5], *pick(normals, P[6:9]),
                                                             pick(tcov, P[10]), 0))
        st = self.gpu.align_settings(**settings)
        g = None if guess is None else (C.c_double * 16)(*guess)
        out, lin = self.outputs()
        if null_output is not None:                                  # 0: the align entry's `out`; 0-3: H, b, error, count
            out[0] = None
            lin[null_output] = None
        rc = self.lib.fdm_cloud_register(method, clouds, g, C.byref(st), 0, *out)
        said = self.lib.fdm_last_error().decode()
        rc2 = self.lib.fdm_cloud_register_linearize(method, clouds, g, C.byref(st), 0, *lin, None)
        assert (rc2, self.lib.fdm_last_error().decode()) == (rc, said)
        return rc, said


def test_every_refusal_says_why_and_the_first_fault_in_the_documented_order_wins(gpu):
    """fdm_last_error() after every refusal of both cloud entries, and where two faults meet the earlier of: null clouds,
    method, robust_kernel, max_correspondence_dist, transform, source cloud, target cloud, (the empty return), plane
    normals, GICP source covariances, GICP target covariances — then the device's own: source, target not finite."""
    call, INVALID = RawEntries(gpu), gpu.capi.FDM_ERR_INVALID
    refused = lambda key, **kw: call(**kw) == (INVALID, MSG[key])       # noqa: E731
    bad_T = np.eye(4).reshape(16).copy()
    bad_T[7] = np.inf
    assert call(0)[0] == 0 and call(1)[0] == 0 and call(2)[0] == 0
    assert refused("null", clouds=None)
    assert refused("method", method=3) and refused("method", method=-1)
    assert refused("kernel", robust_kernel=4) and refused("kernel", robust_kernel=-1)
    assert refused("max_dist", max_correspondence_dist=-1.0) and refused("max_dist", max_correspondence_dist=math.nan)
    assert refused("transform", guess=bad_T)
    assert refused("count", ns=1 << 31) and refused("count", nt=1 << 31)
    assert refused("array", sx=None) and refused("array", tx=None)
    assert refused("normals", method=1, normals=(None, None, None)) and refused("normals", method=1, normals=(call.P[6], None, call.P[8]))
    assert refused("source_cov", method=2, scov=None) and refused("target_cov", method=2, tcov=None)
    assert refused("source_finite", sx=call.dirty(0)) and refused("source_finite", sx=call.dirty(0, -np.inf))
    assert refused("target_finite", tx=call.dirty(3)) and refused("target_finite", tx=call.dirty(3, np.inf))
    # two faults at once
    assert refused("null", clouds=None, method=7, robust_kernel=4)
    assert refused("method", method=3, robust_kernel=4)
    assert refused("kernel", robust_kernel=4, max_correspondence_dist=-1.0)
    assert refused("max_dist", max_correspondence_dist=-1.0, guess=bad_T)
    assert refused("transform", guess=bad_T, sx=None)
    assert refused("count", ns=1 << 31, tx=None)                     # the source cloud, then the target
    assert refused("array", tx=None, method=1, normals=(None, None, None))
    assert refused("source_cov", method=2, scov=None, tcov=None)
    assert refused("source_finite", sx=call.dirty(0), tx=call.dirty(3))
    # an empty cloud returns before the channels are asked for
    assert call(1, nt=0, normals=(None, None, None))[0] == 0 and call(2, ns=0, scov=None, tcov=None)[0] == 0


def test_a_null_output_is_refused_before_anything_else_is_looked_at(gpu):
    """out of fdm_cloud_register, and each of H, b, error and num_inliers of fdm_cloud_register_linearize: `null argument`,
    whatever else is wrong with the call (here an unknown method, which is otherwise the first thing said)."""
    call, INVALID = RawEntries(gpu), gpu.capi.FDM_ERR_INVALID
    assert call(method=7) == (INVALID, MSG["method"])
    for k in range(4):
        assert call(null_output=k) == (INVALID, MSG["null"])
        assert call(method=7, robust_kernel=4, null_output=k) == (INVALID, MSG["null"])


def test_nobody_corresponds_on_the_device(gpu):
    """linearize against an empty target with torch tensors: the correspondences come back as a device tensor of -1 (the
    fill runs on the device), the sums are zero."""
    import torch
    s = [to_device(v) for v in RC.sphere(63)]
    e = [torch.zeros(0, dtype=torch.float32, device=s[0].device) for _ in range(3)]
    lin = gpu.linearize("icp", *s, *e, return_correspondences=True)
    corr = lin["corr"]
    assert torch.is_tensor(corr) and corr.device == s[0].device and corr.dtype == torch.int32 and corr.shape == (63,)
    assert bool((corr == -1).all())
    assert lin["num_inliers"] == 0 and lin["error"] == 0.0 and not lin["H"].any() and not lin["H_upper"].any() and not lin["b"].any()
    assert gpu.register_last_stats()["linearizations"] == 0


def test_python_entries_numpy_and_torch(gpu):
    case = RC.align_case("plane_icp")
    want = case.restated("forward")
    a = align(gpu, case.problem)
    b = align(gpu, case.problem, on_device=True)
    assert isinstance(a, gpu.RegistrationResult) and a.transform.shape == (4, 4) and a.success()
    assert same_bits(a.transform, b.transform) and a.iterations == b.iterations == want.iterations
    assert a.information_matrix() is None or a.information_matrix().shape == (6, 6)
    normals = tuple(case.problem.raw["target_normals"][:, k] for k in range(3))        # three arrays instead of (n, 3)
    c = gpu.align_plane_icp(*case.problem.s, *case.problem.t, normals)
    assert same_bits(a.transform, c.transform)
    with pytest.raises(TypeError):
        gpu.align_icp(*case.problem.s, *case.problem.t, no_such_setting=1)
