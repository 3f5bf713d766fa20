"""Plain NumPy restatement of nanoPCL's k-NN normal and covariance estimation, written from the reference's sources and
not from the engine — the reading fdm_cloud_estimate_normals is held to bit for bit (tests/test_normals_gpu.py); its own
known answers are in tests/test_normal_restate.py.  Test data, not product.

  estimate   geometry::estimateNormals / estimateCovariances / estimateNormalsCovariances
             normal_estimation.hpp:43-63, 107-124, 159-179; impl/normal_estimation_impl.hpp:33-68;
             impl/pca.hpp:34-107; impl/setters.hpp:20-105; search/impl/kdtree_impl.hpp:76-94

Neighbours: brute force over every pair in fp32, ((dx*dx) + (dy*dy)) + (dz*dz) with d = query - point, the query itself a
candidate; the effective_k = min(size_t(k), n) smallest by (d2, input index), in that order.  The index tie-break is this
project's definition (nanoflann's order among equal distances follows its tree).  Sums: sequential fp32 over the
neighbours in order.  The trace test and computeDirect are the oracle's restatement (fdm_ref_post.hpp, computeDirect3)
with trig mode 1 — atan2, sin and cos evaluated in double and rounded once, which is what the device does.
ASSUMED evaluation orders: (sum sumT) * inv_n before the subtraction; every three-term dot
a0 b0 + (a1 b1 + a2 b2); V diag(1e-3, 1, 1) evaluated before the product with VT.
"""
import numpy as np

F32 = np.float32
MAX_K = 64
MIN_NEIGHBORS = 3
GICP_EPSILON = F32(1e-3)
EPS = np.finfo(F32).eps


def effective_k(n, k):
    """min(size_t(k), n): a negative int converts to a huge size_t."""
    return n if k < 0 else min(int(k), n)


def neighbours(x, y, z, k_eff, rows, cells=1 << 23):
    """int64[len(rows), k_eff]: the k_eff points smallest by (d2, index) for the queries `rows`, in that order."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    rows = np.asarray(rows, dtype=np.int64)
    n = x.size
    index = np.arange(n, dtype=np.uint64)
    out = np.empty((rows.size, k_eff), dtype=np.int64)
    chunk = max(1, cells // max(1, n))
    for a in range(0, rows.size, chunk):
        r = rows[a:a + chunk]
        with np.errstate(over="ignore"):
            dx = x[r, None] - x[None, :]
            dy = y[r, None] - y[None, :]
            dz = z[r, None] - z[None, :]
            d2 = ((dx * dx) + (dy * dy)) + (dz * dz)                 # float32 throughout: one rounding per operation
        assert d2.dtype == F32
        # d2 >= +0, so its bits order it: (d2, index) as one integer
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[None, :]
        best = np.sort(np.partition(key, k_eff - 1, axis=1)[:, :k_eff], axis=1)
        out[a:a + chunk] = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return out


def covariances_of(x, y, z, idx):
    """float32[m, 3, 3]: computeMeanAndCovariance (pca.hpp:34-58) over each row of neighbour indices, in order."""
    P = np.stack([np.asarray(v, dtype=F32) for v in (x, y, z)], axis=1)
    m, k = idx.shape
    off = P[idx[:, 0]]
    s = np.zeros((m, 3), dtype=F32)
    q = np.zeros((m, 3, 3), dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(k):
            d = P[idx[:, j]] - off
            s = s + d
            q = q + d[:, :, None] * d[:, None, :]
        inv_n = F32(1.0) / F32(k)
        cov = (q - (s[:, :, None] * s[:, None, :]) * inv_n) * inv_n
    assert cov.dtype == F32
    return cov


def dot3(a, b):
    """a0 b0 + (a1 b1 + a2 b2) along the last axis, fp32."""
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def estimate(x, y, z, k=20, viewpoint=(0.0, 0.0, 0.0), rows=None, idx=None, R=None, setter="both"):
    """estimateNormalsCovariances; setter "normal" / "covariance": estimateNormals / estimateCovariances, which leave the
    other channel at its invalid value here (the reference does not create it).
    (normals float32[m, 3], cov float32[m, 3, 3] indexed [row][column], invalid bool[m]) for the queries `rows` (every
    point if None).  The normals are estimateNormals', the covariances estimateCovariances'; the single pass computes
    the same two from one PCA.  viewpoint None: column 0 as the solver leaves it, not turned (for tests of the
    orientation rule).  idx: neighbours(...) of the rows if the caller has them.  R: the oracle module (fdm_ref_py);
    imported if not given."""
    if R is None:
        import fdm_ref_py as R
    x, y, z = (np.asarray(v, dtype=F32).reshape(-1) for v in (x, y, z))
    n = x.size
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    m = rows.size
    normals = np.zeros((m, 3), dtype=F32)                            # setInvalid: zero normal, identity covariance
    cov = np.tile(np.eye(3, dtype=F32), (m, 1, 1))
    invalid = np.ones(m, dtype=bool)
    k_eff = effective_k(n, k)
    if k_eff < MIN_NEIGHBORS or m == 0:
        return normals, cov, invalid
    if idx is None:
        idx = neighbours(x, y, z, k_eff, rows)
    assert idx.shape == (m, k_eff)
    C = covariances_of(x, y, z, idx)
    with np.errstate(over="ignore", invalid="ignore"):
        trace = (C[:, 0, 0] + C[:, 1, 1]) + C[:, 2, 2]
    ok = np.flatnonzero(~(trace < EPS))                              # computePCA: trace < epsilon is degenerate
    V = np.zeros((m, 3, 3), dtype=F32)
    R.set_trig_mode(1)
    try:
        for i in ok:
            V[i] = R.eig3(C[i])[1]                                   # columns = eigenvectors, eigenvalues ascending
    finally:
        R.set_trig_mode(0)
    Vk = V[ok]
    P = np.stack([x, y, z], axis=1)[rows[ok]]
    invalid[ok] = False
    nrm = Vk[:, :, 0]
    if setter == "covariance":
        pass
    elif viewpoint is None:
        normals[ok] = nrm
    else:
        vp = np.asarray(viewpoint, dtype=F32)
        flip = dot3(nrm, vp[None, :] - P) < 0                        # exactly 0 does not flip
        normals[ok] = np.where(flip[:, None], -nrm, nrm)
    if setter != "normal":
        W = Vk * np.array([GICP_EPSILON, 1.0, 1.0], dtype=F32)[None, None, :]   # V's columns scaled first
        cov[ok] = dot3(W[:, :, None, :], Vk[:, None, :, :])          # C(r, c) = sum_j W(r, j) V(c, j)
    assert normals.dtype == F32 and cov.dtype == F32
    return normals, cov, invalid


def kth_distance(x, y, z, k_eff, rows):
    """float32[len(rows)]: the distance to the k_eff-th neighbour (the query itself is the first)."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    idx = neighbours(x, y, z, k_eff, rows)[:, -1]
    rows = np.asarray(rows, dtype=np.int64)
    d = np.stack([x[rows] - x[idx], y[rows] - y[idx], z[rows] - z[idx]], axis=1).astype(np.float64)
    return np.sqrt((d * d).sum(axis=1))
