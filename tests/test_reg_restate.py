"""The NumPy restatement of nanoPCL's registration (tests/reg_restate.py) against the reference's own known answers
(lib/nanoPCL/tests/test_registration.cpp, groups A, B and C) at its own tolerances, the admission of the align cases the
device is held to (tests/reg_cases.py), and the host algebra of the engine (fastdem_amd/csrc/fdm_register_host.hpp) against
the restatement in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import reg_cases as RC
import reg_restate as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- A. components ----
def test_lie_exp_log_round_trip():
    xi = np.array([0.01, 0.02, 0.03, 0.1, 0.2, 0.15])
    assert np.abs(RR.se3_log(RR.se3_exp(xi)) - xi).max() < 1e-10
    small = np.array([1e-5, 2e-5, 3e-5, 1e-4, 2e-4, 1e-4])
    assert np.abs(RR.se3_log(RR.se3_exp(small)) - small).max() < 1e-12
    assert np.linalg.norm(RR.se3_exp(np.zeros(6)) - np.eye(4)) < 1e-15


def test_se3_exp_is_a_rigid_transform_with_the_twist_laid_out_v_then_omega():
    T = RR.se3_exp([1.0, 2.0, 3.0, 0.0, 0.0, 0.0])
    assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], [1.0, 2.0, 3.0])
    T = RR.se3_exp([0.0, 0.0, 0.0, 0.0, 0.0, math.pi / 2])
    assert np.abs(T[:3, :3] - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() < 1e-15
    R = RR.so3_exp([0.3, -0.2, 0.5])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
    assert np.array_equal(RR.so3_exp([5e-11, 0, 0]), np.eye(3))      # below 1e-10: the identity


def test_robust_weights():
    w = RR.robust_weight
    assert abs(w(0.1, RR.HUBER, 1.0) - 1.0) < 1e-10 and w(0.1, RR.HUBER, 1.0) > w(2.0, RR.HUBER, 1.0) == 0.5
    assert w(0.1, RR.CAUCHY, 1.0) > w(5.0, RR.CAUCHY, 1.0) == 1.0 / 26.0
    assert w(0.1, RR.TUKEY, 1.0) > 0 and abs(w(2.0, RR.TUKEY, 1.0)) < 1e-10
    assert w(0.5, RR.TUKEY, 1.0) == 0.5625
    assert abs(w(0.1, RR.NONE, 1.0) - 1.0) < 1e-10 and abs(w(100.0, RR.NONE, 1.0) - 1.0) < 1e-10


def test_quadratic_model_packing():
    H = RR.full_hessian(np.arange(1.0, 22.0))
    assert H[0, 1] == H[1, 0] and H[2, 5] == H[5, 2]
    assert (H[0, 0], H[1, 1], H[5, 5]) == (1.0, 7.0, 21.0)


def test_regularize():
    eps = 1e-3
    v = np.array([1.0, 2.0, -2.0]) / 3.0
    Vfull = np.linalg.qr(np.stack([v, [0, 1, 1], [1, 0, 0]], axis=1))[0]
    C = (Vfull @ np.diag([1e-3, 1.0, 1.0]) @ Vfull.T).astype(np.float32)
    out = RR.regularize(np.stack([C, np.eye(3, dtype=np.float32), np.full((3, 3), np.nan, dtype=np.float32),
                                  np.diag([1.0, 0.5, 1.0]).astype(np.float32)]), eps)
    w = np.linalg.eigvalsh(out[0])
    assert np.abs(w - [eps, 1, 1]).max() < 1e-12 and np.abs(out[0] @ Vfull[:, 0] - eps * Vfull[:, 0]).max() < 1e-6
    # the identity of an invalid point (ASSUMED); 1 - (1 - eps) is eps to one rounding
    assert np.abs(out[1] - np.diag([eps, 1.0, 1.0])).max() < 1e-18 + 2.0 ** -53
    assert np.array_equal(out[2], np.eye(3) * eps)                   # cov(0, 0) not finite
    assert np.abs(out[3] - np.diag([1.0, eps, 1.0])).max() < 1e-18 + 2.0 ** -53


def test_factors_against_their_jacobians():
    """H = JT W J, b = JT W r, e = rT W r / 2 with J = [I, -[p]x].  The ICP factor's off-diagonal block is kept AS WRITTEN
    in icp_factor.hpp:63-71 — rows (-z, y, 0), (z, 0, -x), (-y, x, 0), which is not -[p]x — so only its other blocks,
    b and e are held to J; the GICP factor with W = I has the block J gives."""
    p, q = np.array([[0.3, -1.2, 2.0]]), np.array([[0.1, -1.0, 2.5]])
    S = RR.terms("icp", p, q)[0]
    J = np.hstack([np.eye(3), -RR.skew(p[0])])
    r = p[0] - q[0]
    H, want = RR.full_hessian(S[:21]), J.T @ J
    assert np.abs(H[:3, :3] - want[:3, :3]).max() < 1e-15 and np.abs(H[3:, 3:] - want[3:, 3:]).max() < 1e-15
    assert np.array_equal(H[:3, 3:], [[-2.0, -1.2, 0.0], [2.0, 0.0, -0.3], [1.2, 0.3, 0.0]])
    assert np.abs(S[21:27] - J.T @ r).max() < 1e-15 and abs(S[27] - 0.5 * r @ r) < 1e-16
    n = np.array([[0.0, 0.6, 0.8]])
    S = RR.terms("plane", p, q, RR.NONE, 1.0, normals=n)[0]
    Jp = (n[0] @ J)[None, :]
    assert np.abs(RR.full_hessian(S[:21]) - Jp.T @ Jp).max() < 1e-15 and abs(S[27] - 0.5 * (n[0] @ r) ** 2) < 1e-16
    C = np.eye(3)[None] * 0.5
    S = RR.terms("gicp", p, q, RR.NONE, 1.0, R=np.eye(3), Cs=C, Ct=C)[0]   # W = I: the ICP factor
    assert np.abs(RR.full_hessian(S[:21]) - J.T @ J).max() < 1e-14 and abs(S[27] - 0.5 * r @ r) < 1e-15


def test_nearest_takes_the_lower_index_and_the_radius_is_inclusive():
    t = [np.array(v, dtype=np.float32) for v in ([1.0, -1.0, 3.0], [0, 0, 0], [0, 0, 0])]
    p = np.array([[0.0, 0.0, 0.0], [0.75, 0.0, 0.0]])
    assert RR.correspondences(p, *t, 1.0).tolist() == [0, 0]
    assert RR.correspondences(p, t[0][::-1], t[1], t[2], 1.0).tolist() == [1, 2]
    assert RR.correspondences(p, *t, np.nextafter(np.float32(1.0), np.float32(0))).tolist() == [-1, 0]


# ---- B, C. the convergence and stability cases, and their admission ----
@pytest.mark.parametrize("name", RC.ALIGN_CASES)
def test_align_cases_meet_the_reference_tolerances_and_are_admitted(name):
    case = RC.align_case(name)
    runs = [case.restated(order) for order in ("forward", "reversed", "pairwise")]
    a = runs[0]
    spread = max(float(np.linalg.norm(r.transform - a.transform)) for r in runs[1:])
    err = RR.transform_error(a.transform, case.gt) if case.gt is not None else float("nan")
    print(f"{name}: iterations {a.iterations}, converged {a.converged}, inliers {a.num_inliers}/{case.problem.n}, fitness "
          f"{a.fitness:.4f}, rmse {a.rmse:.3e}, error to truth {err:.3e}, spread {spread:.3e} (recorded {case.spread:.1e})")
    for r in runs[1:]:
        assert (r.iterations, r.converged, r.num_inliers) == (a.iterations, a.converged, a.num_inliers)
    assert spread <= 4.0 * case.spread            # (the record is the measurement; the factor is this check's own allowance)
    if case.tol is not None:
        assert a.converged and err < case.tol
    if name == "partial_overlap":
        assert a.fitness < 1.0
    if name == "sparse":
        assert not a.converged and a.iterations == 0 and a.fitness == 0.0 and math.isinf(a.rmse)
    if name == "perfect_plane":
        assert a.converged and a.covariance is None
        assert not a.H[0].any() and not a.H[1].any() and not a.H[5].any()
    if name in RC.SPHERE_CASES:
        assert a.covariance is not None
    if name.startswith("icp_max_iterations"):
        assert not a.converged and a.iterations == int(name[-1])


def test_empty_clouds_and_no_iterations():
    e = tuple(np.zeros(0, dtype=np.float32) for _ in range(3))
    guess = RC.translation(1.0, 2.0, 3.0)
    for s, t in ((e, RC.sphere(100)), (RC.sphere(100), e)):
        r = RR.align(RR.Problem("icp", s, t), guess)
        assert not r.converged and r.iterations == 0 and r.fitness == 0.0 and math.isinf(r.rmse)
        assert r.covariance is None and np.array_equal(r.transform, guess)
    c = RC.sphere(100)
    r = RR.align(RR.Problem("icp", c, c, max_iterations=0), guess)
    assert not r.converged and r.iterations == 0 and r.fitness == 0.0 and math.isinf(r.rmse) and r.covariance is None
    assert np.array_equal(r.transform, guess)


def test_the_eps_names_are_swapped_as_in_the_reference():
    delta = np.array([1e-3, 0, 0, 0, 0, 1e-6])                      # |v| = 1e-3, |omega| = 1e-6
    assert RR.converged(delta, 1.0, 0.5, translation_eps=1e-5, rotation_eps=1e-2, relative_error_eps=0.0)
    assert not RR.converged(delta, 1.0, 0.5, translation_eps=1e-2, rotation_eps=1e-5, relative_error_eps=0.0)
    assert RR.converged(np.ones(6), 1.0, 1.0 - 1e-7, 0.0, 0.0, 1e-6)     # stalled
    assert RR.converged(np.ones(6), 0.0, 5.0, 0.0, 0.0, 1e-6)            # prev_error 0: rel_change 0


# ---- the engine's host algebra, stand-alone and sanitized ----
PROBE = os.path.join(ROOT, "fastdem_amd", "cpp", "tests", "reg_host_probe.cpp")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("reg_host") / "reg_host_probe")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "fastdem_amd", "csrc"), PROBE, "-o", exe])

    def run(*numbers):
        text = " ".join(float(v).hex() for v in numbers)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return [float.fromhex(tok) for tok in r.stdout.split()]
    return run


def spd(seed, scale=1.0):
    g = np.random.default_rng(seed)
    J = g.normal(size=(40, 6)) * np.array([1, 1, 1, scale, scale, scale])
    return J.T @ J, g.normal(size=6)


def upper(H):
    return H[np.triu_indices(6)]


def test_host_algebra_solve_exp_criteria_and_cholesky_rule(probe):
    # op 1: delta = (H + lambda I)^-1 (-b) and new_T = se3Exp(delta) * T
    for seed, scale in ((1, 1.0), (2, 30.0), (3, 1e-3)):
        H, b = spd(seed, scale)
        T = RC.random_transform(0.3, 0.15, seed)
        out = probe(1, *upper(H), *b, *T.T.reshape(16))
        delta, new_T = np.array(out[:6]), np.array(out[6:22]).reshape(4, 4).T
        want = RR.compute_delta(H, b)
        cond = np.linalg.cond(H + RR.LAMBDA * np.eye(6))
        assert np.abs(delta - want).max() <= 64 * cond * 2.0 ** -53 * np.abs(want).max()
        assert np.abs(new_T - RR.rigid_mul(RR.se3_exp(delta), T)).max() <= 8 * 2.0 ** -53 * max(1.0, np.abs(new_T).max())
    # op 2: se3Exp alone, the small-angle branch included
    for xi in ([0.01, 0.02, 0.03, 0.1, 0.2, 0.15], [1, 2, 3, 5e-11, 0, 0], [1, 2, 3, 2e-10, 0, 0], [0, 0, 0, 0, 3.0, 0]):
        got = np.array(probe(2, *xi)).reshape(4, 4).T
        assert np.abs(got - RR.se3_exp(xi)).max() <= 4 * 2.0 ** -53 * 4.0
    # op 3: the criteria, names as in the reference
    for args in ((1e-3, 0, 0, 0, 0, 1e-6, 1.0, 0.5, 1e-5, 1e-2, 0.0), (1e-3, 0, 0, 0, 0, 1e-6, 1.0, 0.5, 1e-2, 1e-5, 0.0),
                 (1, 1, 1, 1, 1, 1, 1.0, 1.0 - 1e-7, 0.0, 0.0, 1e-6), (1, 1, 1, 1, 1, 1, 0.0, 5.0, 0.0, 0.0, 1e-6),
                 (1, 1, 1, 1, 1, 1, np.finfo(float).max, 5.0, 1e-4, 1e-4, 1e-6)):
        assert bool(probe(3, *args)[0]) == RR.converged(np.array(args[:6]), *args[6:])
    # op 4: the covariance and its rule
    H, _ = spd(4)
    out = probe(4, 1000, *upper(H))
    assert out[0] == 1.0
    assert np.abs(np.array(out[1:]).reshape(6, 6) - np.linalg.inv(H)).max() <= 64 * np.linalg.cond(H) * 2.0 ** -53 * np.abs(np.linalg.inv(H)).max()
    J = np.random.default_rng(5).normal(size=(40, 6))
    J[:, 5] = 0.0                                                    # a zero row and column: semidefinite
    assert probe(4, 1000, *upper(J.T @ J))[0] == 0.0 and RR.covariance_of(J.T @ J, 1000) is None
    J[:, 5] = J[:, 4] * (1 + 1e-9)                                   # rank 5 up to 1e-9: below the floor at n = 1000
    Hs = J.T @ J
    assert probe(4, 1000, *upper(Hs))[0] == (0.0 if RR.covariance_of(Hs, 1000) is None else 1.0) == 0.0
    assert probe(4, 1000, *np.zeros(21))[0] == 0.0
