"""The clouds and cases of the registration tests (tests/test_reg_restate.py on the CPU, tests/test_register_gpu.py on the
device), of the construction the reference's own tests use (lib/nanoPCL/tests/test_registration.cpp): points on the unit
sphere, the noisy plane z = 0.1 x + 0.2 y +- 0.01, transforms up to 0.3 m / 0.15 rad.  NumPy's generator, not libstdc++'s
stream.  Normals and covariances come from tests/normal_restate.py.  Everything is computed once and shared; the arrays
are read-only.

ALIGN CASES.  Each carries the reference's tolerance against its ground truth (`tol`, None where the reference only looks
at a flag) and SPREAD: the largest Frobenius difference between the transforms the restatement's align reaches when it sums
the per-point terms forward, reversed and pairwise.  A case is admitted only if iterations, converged and num_inliers
agree across the three (tests/test_reg_restate.py asserts that, and that the spread it measures is within four times what
is recorded here — the allowance is for another build of NumPy's 6 x 6 solve and is the CPU check's alone); the device,
whose sums have yet another order, is held to 64 x SPREAD with a floor of 1e-13.
"""
import functools
import math

import numpy as np

import normal_restate as NR
import reg_restate as RR

F32 = np.float32


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def sphere(n, seed=42, radius=1.0):
    """createRandomSphere: (x, y, z) float32."""
    g = np.random.default_rng(seed)
    p = g.uniform(-1.0, 1.0, size=(n, 3)).astype(F32)
    norm = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])
    small = norm < F32(1e-6)
    p[small, 0], norm[small] = 1.0, 1.0
    p = F32(radius) * p / norm[:, None]
    return frozen(*(np.ascontiguousarray(p[:, a], dtype=F32) for a in range(3)))


@functools.lru_cache(maxsize=None)
def plane(n, seed=42):
    """createRandomPlane: z = 0.1 x + 0.2 y + noise, x, y in +-5, noise in +-0.01."""
    g = np.random.default_rng(seed)
    x = g.uniform(-5.0, 5.0, n).astype(F32)
    y = g.uniform(-5.0, 5.0, n).astype(F32)
    z = F32(0.1) * x + F32(0.2) * y + F32(0.0) + g.uniform(-0.01, 0.01, n).astype(F32)
    return frozen(x, y, z.astype(F32))


def random_transform(max_t, max_r, seed=123):
    """createRandomTransform: a translation in +-max_t per axis, a rotation about a random axis by its length."""
    g = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, 3] = g.uniform(-max_t, max_t, 3)
    axis = g.uniform(-max_r, max_r, 3)
    if np.linalg.norm(axis) > 1e-6:
        T[:3, :3] = RR.so3_exp(axis)
    return T


def translation(x, y, z):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def transform_cloud(cloud, T):
    """transformCloud: the points through T, rounded to float32."""
    p = RR.transform_points(T, *cloud).astype(F32)
    return frozen(*(np.ascontiguousarray(p[:, a]) for a in range(3)))


@functools.lru_cache(maxsize=None)
def _oracle():
    import fdm_ref_py
    fdm_ref_py.load()
    return fdm_ref_py


_NC = {}


def normals_covariances(cloud, k=20):
    """(normals float32[n, 3], covariances float32[n, 3, 3]) of estimateNormalsCovariances(cloud, k); kept per cloud."""
    key = (cloud[0].tobytes(), cloud[1].tobytes(), cloud[2].tobytes(), k)
    if key not in _NC:
        normals, cov, _ = NR.estimate(*cloud, k, R=_oracle())
        _NC[key] = frozen(normals, cov)
    return _NC[key]


# ---- align cases ----
# The measurements of tests/test_reg_restate.py (it prints them), as measured, rounded up in the second digit.  A
# converged fixed point forgets the order of the sums; only the case that does not settle shows it.
SPREAD = {
    "icp_identity": 0.0, "icp_translation": 1.4e-17, "icp_rotation_translation": 1.4e-16, "plane_icp": 1.7e-15,
    "gicp": 3.2e-16, "gicp_identity": 0.0, "partial_overlap": 5.1e-14, "sparse": 0.0, "perfect_plane": 1.9e-18,
    "icp_max_iterations_1": 5.5e-17, "icp_max_iterations_2": 7.1e-17,
}


class Case:
    def __init__(self, name, problem, gt=None, tol=None, guess=None):
        self.name, self.problem, self.gt, self.tol, self.guess = name, problem, gt, tol, guess
        self.spread = SPREAD[name]

    @functools.lru_cache(maxsize=None)
    def restated(self, order="forward"):
        return RR.align(self.problem, self.guess, order)


@functools.lru_cache(maxsize=None)
def align_case(name):
    if name == "icp_identity":
        c = sphere(500)
        return Case(name, RR.Problem("icp", c, c), np.eye(4), 1e-6)
    if name == "icp_translation":
        t = sphere(500)
        gt = translation(0.5, 0.0, 0.0)
        return Case(name, RR.Problem("icp", transform_cloud(t, np.linalg.inv(gt)), t, max_iterations=100), gt, 0.01)
    if name in ("icp_rotation_translation", "icp_max_iterations_1", "icp_max_iterations_2"):
        t = sphere(1000)
        gt = random_transform(0.3, 0.15, 42)
        it = {"icp_rotation_translation": 100, "icp_max_iterations_1": 1, "icp_max_iterations_2": 2}[name]
        return Case(name, RR.Problem("icp", transform_cloud(t, np.linalg.inv(gt)), t, max_iterations=it), gt,
                    0.05 if it == 100 else None)
    if name == "plane_icp":
        t = plane(1000)
        gt = random_transform(0.2, 0.1, 42)
        return Case(name, RR.Problem("plane", transform_cloud(t, np.linalg.inv(gt)), t,
                                     target_normals=normals_covariances(t)[0]), gt, 0.02)
    if name == "gicp":
        t = sphere(1000)
        gt = random_transform(0.2, 0.1, 42)
        s = transform_cloud(t, np.linalg.inv(gt))
        return Case(name, RR.Problem("gicp", s, t, source_cov=normals_covariances(s)[1],
                                     target_cov=normals_covariances(t)[1]), gt, 0.02)
    if name == "gicp_identity":
        c = sphere(500)
        cov = normals_covariances(c)[1]
        return Case(name, RR.Problem("gicp", c, c, source_cov=cov, target_cov=cov), np.eye(4), 1e-5)
    if name == "partial_overlap":
        t = sphere(500, 42)
        s = transform_cloud(sphere(500, 43), translation(1.5, 0.0, 0.0))
        # Three iterations, not the reference's 50: the 1.5 m shift leaves a quarter of the source within 0.3 m and ICP
        # does not settle on it — the three summation orders drift apart by a factor of about ten per iteration
        # (5e-14 after 3, 3e-12 after 5, 2e-9 after 8, 1e-5 after 12, different inlier counts after 50), a decision
        # boundary at every step.  What the reference asserts, fitness < 1, holds from the first iteration on.
        return Case(name, RR.Problem("icp", s, t, max_correspondence_dist=0.3, max_iterations=3))
    if name == "sparse":
        s = tuple(np.array(v, dtype=F32) for v in ([0, 1, 0], [0, 0, 1], [0, 0, 0]))
        t = tuple(np.array(v, dtype=F32) for v in ([0.1, 1.1, 0.1], [0, 0, 1], [0, 0, 0]))
        return Case(name, RR.Problem("icp", s, t, min_correspondences=10))
    if name == "perfect_plane":
        # the plane z = 0 with the exact normal (0, 0, 1): the rows of H for x, y and yaw are exactly zero
        g = np.random.default_rng(7)
        t = frozen(g.uniform(-5, 5, 600).astype(F32), g.uniform(-5, 5, 600).astype(F32), np.zeros(600, dtype=F32))
        nrm = np.tile(np.array([0, 0, 1], dtype=F32), (600, 1))
        gt = RR.se3_exp([0.0, 0.0, 0.05, 0.01, -0.02, 0.0])
        return Case(name, RR.Problem("plane", transform_cloud(t, np.linalg.inv(gt)), t, target_normals=nrm), gt)
    raise KeyError(name)


ALIGN_CASES = ("icp_identity", "icp_translation", "icp_rotation_translation", "plane_icp", "gicp", "gicp_identity",
               "partial_overlap", "sparse", "perfect_plane", "icp_max_iterations_1", "icp_max_iterations_2")
SPHERE_CASES = ("icp_translation", "icp_rotation_translation", "gicp")   # the covariance is checked on these


# ---- linearize cases: two samples of the sphere, 0.1 apart at the most, so that the inliers are a proper subset ----
LIN_SOURCE_SIZES = (1, 63, 64, 65, 256, 257, 769, 1000)   # with 1 000 target points
LIN_TARGET_SIZES = (1, 2, 257, 1000)                      # with 257 source points
LIN_WIDTH = {"icp": 1.0, "plane": 0.002, "gicp": 0.03}       # of the size of the residuals, so that every kernel bites


@functools.lru_cache(maxsize=None)
def lin_base():
    s, t = sphere(1000, 43), sphere(1000, 42)
    (sn, sc), (tn, tc) = normals_covariances(s), normals_covariances(t)
    return s, t, sc, tn, tc


def lin_transforms():
    return (np.eye(4), random_transform(0.02, 0.03, 5), random_transform(0.05, 0.1, 6))


@functools.lru_cache(maxsize=None)
def lin_problem(method, kernel, ns, nt):
    s, t, sc, tn, tc = lin_base()
    cut = lambda c, n: tuple(v[:n] for v in c)   # noqa: E731
    return RR.Problem(method, cut(s, ns), cut(t, nt), target_normals=tn[:nt] if method == "plane" else None,
                      source_cov=sc[:ns] if method == "gicp" else None, target_cov=tc[:nt] if method == "gicp" else None,
                      max_correspondence_dist=0.1, robust_kernel=kernel, robust_kernel_width=LIN_WIDTH[method])


def lin_shapes():
    return [(ns, 1000) for ns in LIN_SOURCE_SIZES] + [(257, nt) for nt in LIN_TARGET_SIZES]


def ring_limit(gx, gy, h, max_dist):
    """The ring limit the host sets (the walk's bound at margin 0, in float32, capped by the grid)."""
    cap = max(gx, gy) - 1
    h = F32(h)
    max_d2 = F32(max_dist) * F32(max_dist)
    for s in range(cap):
        lb = ((F32(s) - F32(0.00390625)) * h) * F32(0.9999)
        if lb > 0 and max_d2 < (lb * lb) * F32(0.9999):
            return s
    return cap


def bound(n, abs_sums):
    """(2 n + 32) 2^-53 sum|term|: two summations of n doubles and a few roundings per term."""
    return (2 * n + 32) * 2.0 ** -53 * abs_sums


assert math.isfinite(sum(SPREAD.values()))
