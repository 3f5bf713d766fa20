"""The clouds and cases of the voxelized-GICP tests (tests/test_vgicp_restate.py on the CPU, tests/test_vgicp_gpu.py on the
device).  NumPy's generator, not libstdc++'s stream; source covariances from tests/normal_restate.py with k = 20.
Everything is computed once and shared; the arrays are read-only.

THE DESIGNED CLOUD.  Per-voxel eigen-gaps of random clouds are small (a 5 000-point radius-5 sphere at 0.5 m: smallest
relative gap (l1 - l0) / l2 among full voxels 2.4e-5), and two double eigen-solvers disagree by about eps / gap in v0, so
such clouds cannot hold a regularised covariance to 1e-12.  designed() builds one small disc per occupied voxel instead:
edge 0.5, cells drawn without repetition from a 24^3 block around the origin (negative indices included, so that floor
matters); a full voxel gets m points on a randomly oriented plane through the voxel centre at angles 2 pi k / m + one
random phase, radii 0.15-0.3 of the edge, thickness +-0.01 of the edge; a sparse voxel 1 or 2 uniform points within +-0.2
of the edge; all points shuffled.  Every test that compares C_reg or sums first asserts, on the restatement alone, that
every full voxel's gap is >= MIN_GAP; if a seed fails that, change the seed, not the limit.

ALIGN CASES.  The reference's own (lib/nanoPCL/tests/test_registration.cpp groups D and E) with its tolerances, and two
on the designed cloud.  SPREAD: as in reg_cases — the largest Frobenius difference between the transforms the restatement
reaches summing forward, reversed and pairwise, as measured by tests/test_vgicp_restate.py (it prints them), rounded up in
the second digit; the device is held to 64 x SPREAD with a floor of 1e-13.
"""
import functools
import math

import numpy as np

import reg_cases as RC
import reg_restate as RR
import vgicp_restate as VG

F32 = np.float32
EDGE = 0.5
MIN_GAP = 0.25
frozen = RC.frozen


@functools.lru_cache(maxsize=None)
def designed(n_voxels, counts=(1, 2, 3, 4, 5, 8, 200), seed=11):
    """(x, y, z) float32: one disc per voxel, the voxels' point counts drawn from `counts`."""
    g = np.random.default_rng(seed)
    cells = g.choice(24 ** 3, size=n_voxels, replace=False)
    idx = np.stack([cells % 24, (cells // 24) % 24, cells // 576], axis=1).astype(np.int64) - 12
    m_of = g.choice(np.asarray(counts), size=n_voxels)
    pts = []
    for c, m in zip(idx, m_of):
        centre = (c.astype(np.float64) + 0.5) * EDGE
        if m < 3:
            pts.append(centre + g.uniform(-0.2, 0.2, size=(m, 3)) * EDGE)
            continue
        nrm = g.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        u = np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        ang = 2.0 * math.pi * np.arange(m) / m + g.uniform(0.0, 2.0 * math.pi)
        rad = g.uniform(0.15, 0.3, size=m) * EDGE
        thick = g.uniform(-0.01, 0.01, size=m) * EDGE
        pts.append(centre + rad[:, None] * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * v) + thick[:, None] * nrm)
    p = np.concatenate(pts).astype(F32)
    p = p[g.permutation(p.shape[0])]
    return frozen(*(np.ascontiguousarray(p[:, a]) for a in range(3)))


@functools.lru_cache(maxsize=None)
def designed_map(n_voxels, counts=(1, 2, 3, 4, 5, 8, 200), seed=11):
    return VG.Map(*designed(n_voxels, counts, seed), EDGE)


def assert_gaps(vmap):
    """The condition of every tight comparison, on the restatement alone."""
    assert vmap.min_gap() >= MIN_GAP, f"smallest relative eigen-gap {vmap.min_gap():.3g} < {MIN_GAP}: change the seed"


@functools.lru_cache(maxsize=None)
def sparse_outdoor(n, seed=42):
    """createSparseOutdoor: x, y in +-50; z = 0.1 sin(0.1 x) with probability 0.7, else uniform in 0 .. 3."""
    g = np.random.default_rng(seed)
    x = g.uniform(-50.0, 50.0, n).astype(F32)
    y = g.uniform(-50.0, 50.0, n).astype(F32)
    ground = g.uniform(0.0, 1.0, n).astype(F32) < F32(0.7)
    h = g.uniform(0.0, 3.0, n).astype(F32)
    z = np.where(ground, F32(0.1) * np.sin(x * F32(0.1)).astype(F32), h).astype(F32)
    return frozen(x, y, z)


def sparse_gt():
    """3 degrees about z, then the translation (0.5, 0.25, 0) in front."""
    T = np.eye(4)
    T[:3, :3] = RR.so3_exp([0.0, 0.0, math.radians(3.0)])
    T[:3, 3] = (0.5, 0.25, 0.0)
    return T


def pose_errors(T, gt):
    """(translation error in metres, rotation error in degrees) of inverse(gt) * T."""
    E = np.linalg.inv(gt) @ T
    c = min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1.0) / 2.0))
    return float(np.linalg.norm(E[:3, 3])), math.degrees(math.acos(c))


# The measurements of tests/test_vgicp_restate.py, rounded up in the second digit.
SPREAD = {
    "identity": 1.9e-17, "convergence": 3.4e-16, "very_sparse": 7.3e-16, "sparse": 1.4e-16, "moderate": 2.6e-16,
    "dense": 5.1e-16, "designed_small": 7.8e-17, "designed_huber": 4.6e-16,
}
SPARSE = {"very_sparse": (500, 2.0, None), "sparse": (1000, 1.5, (0.1, 1.0)), "moderate": (2000, 1.0, (0.05, 0.5)),
          "dense": (5000, 1.0, (0.05, 0.5))}   # points, voxel, the reference's limits (metres, degrees)


class Case:
    def __init__(self, name, source, source_cov, target, resolution, gt, tol=None, limits=None, **settings):
        self.name, self.source, self.source_cov, self.target, self.resolution = name, source, source_cov, target, resolution
        self.gt, self.tol, self.limits, self.settings = gt, tol, limits, settings
        self.spread = SPREAD[name]

    @functools.cached_property
    def map(self):
        return VG.Map(*self.target, self.resolution, self.settings.get("covariance_epsilon", 1e-3))

    @functools.cached_property
    def problem(self):
        return VG.Problem(self.source, self.source_cov, self.map, **self.settings)

    @functools.lru_cache(maxsize=None)
    def restated(self, order="forward"):
        return RR.align(self.problem, None, order)


@functools.lru_cache(maxsize=None)
def align_case(name):
    if name == "identity":
        c = RC.sphere(5000, 42, 5.0)
        return Case(name, c, RC.normals_covariances(c)[1], c, 0.5, np.eye(4), 0.01, max_iterations=30, min_correspondences=5)
    if name == "convergence":
        t = RC.sphere(5000, 42, 5.0)
        gt = RC.random_transform(0.1, 0.05, 42)
        s = RC.transform_cloud(t, np.linalg.inv(gt))
        return Case(name, s, RC.normals_covariances(s)[1], t, 0.5, gt, 0.2, max_iterations=50, min_correspondences=5)
    if name in SPARSE:
        n, voxel, limits = SPARSE[name]
        t = sparse_outdoor(n)
        gt = sparse_gt()
        moved = RC.transform_cloud(t, np.linalg.inv(gt))
        noise = np.random.default_rng(123).normal(0.0, 0.02, size=(n, 3)).astype(F32)
        s = frozen(*(np.ascontiguousarray(moved[a] + noise[:, a]) for a in range(3)))
        return Case(name, s, RC.normals_covariances(s)[1], t, voxel, gt, None, limits, max_iterations=50,
                    min_correspondences=3)
    if name in ("designed_small", "designed_huber"):
        t = designed(300, (1, 2, 3, 4, 5, 8))
        gt = RC.random_transform(0.03, 0.01, 5) if name == "designed_small" else RC.random_transform(0.08, 0.03, 6)
        s = RC.transform_cloud(t, np.linalg.inv(gt))
        extra = {} if name == "designed_small" else {"robust_kernel": "huber", "robust_kernel_width": 0.15}
        return Case(name, s, RC.normals_covariances(s)[1], t, EDGE, gt, None, None, max_iterations=50, **extra)
    raise KeyError(name)


REFERENCE_CASES = ("identity", "convergence", "very_sparse", "sparse", "moderate", "dense")
ALIGN_CASES = REFERENCE_CASES + ("designed_small", "designed_huber")

# ---- linearize cases: the designed cloud against itself moved, so that points cross voxel faces ----
LIN_SOURCE_SIZES = (1, 63, 64, 65, 256, 257, 769, 1000)   # against a 300-voxel map
LIN_WIDTH = 0.2                                            # of the size of the Mahalanobis residuals, so that every kernel bites


@functools.lru_cache(maxsize=None)
def lin_base():
    """(target cloud, its map, source cloud of >= 1 000 points, source covariances)."""
    t = designed(300, (1, 2, 3, 4, 5, 8))
    assert t[0].size >= 1000
    return t, VG.Map(*t, EDGE), RC.normals_covariances(t)[1]


def lin_transforms():
    return (RC.random_transform(0.1, 0.02, 7), RC.random_transform(0.2, 0.05, 8), RC.random_transform(0.3, 0.1, 9))


@functools.lru_cache(maxsize=None)
def lin_problem(kernel, ns):
    t, vmap, cov = lin_base()
    return VG.Problem(tuple(v[:ns] for v in t), cov[:ns], vmap, robust_kernel=kernel, robust_kernel_width=LIN_WIDTH)


bound = RC.bound
assert math.isfinite(sum(SPREAD.values()))
