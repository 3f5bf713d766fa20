"""Plain NumPy restatement of nanoPCL's cloud registration (alignICP, alignPlaneICP, alignGICP), written from the
reference's sources and not from the engine — the reading fdm_cloud_register and fdm_cloud_register_linearize are held to
(tests/test_register_gpu.py); its own known answers are in tests/test_reg_restate.py.  Test data, not product.

  se3_exp, se3_log        core/lie.hpp:39-168 (so3Exp / so3Log through Eigen's AngleAxis)
  robust_weight           registration/factors/robust_kernels.hpp:42-74
  full_hessian            registration/linearizers/linearizer.hpp:42-53
  correspondences         registration/correspondence/kdtree_correspondence.hpp:57-120, search/impl/kdtree_impl.hpp:62-74
  regularize              registration/factors/gicp_factor.hpp:53-65, 215-235
  terms, linearize        registration/factors/{icp,plane,gicp}_factor.hpp, linearizers/linearizer.hpp:120-146
  compute_delta, converged, covariance_of, align
                          optimizers/lm_optimizer.hpp:98-103, criteria.hpp:40-54, iterative_solver.hpp:96-219

p = T * source[i] is ((r0 x + r1 y) + r2 z) + t per row in double (ASSUMED order: DESIGN.md §6), rounded once to float32
for the search; d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float32 with d = p - target; the nearest target is the smallest
(d2, target index) — the index tie-break is this project's definition — accepted iff d2 <= max_dist * max_dist (a float32
product).  The factors are double, operation for operation as the reference writes them.  Sums of the per-point terms:
`order` "exact" (math.fsum, correctly rounded: what the device's sums are measured against), "forward", "reversed" or
"pairwise" (what align's admission runs).  The twist is [v; omega]; criteria.hpp's eps names are swapped relative to it
and are kept as written.  The covariance follows this project's documented rule (include/fdm_engine.h): inverse(H) where
an unpivoted Cholesky finds every pivot above n_source * 2^-52 * max diag(H).
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
NONE, HUBER, TUKEY, CAUCHY = 0, 1, 2, 3
KERNELS = {"none": NONE, "huber": HUBER, "tukey": TUKEY, "cauchy": CAUCHY}
LAMBDA = 1e-3
DBL_MAX = np.finfo(F64).max
DEFAULTS = dict(max_correspondence_dist=1.0, max_iterations=50, translation_eps=1e-4, rotation_eps=1e-4,
                relative_error_eps=1e-6, min_correspondences=10, robust_kernel=NONE, robust_kernel_width=1.0,
                covariance_epsilon=1e-3)


# ---- Lie ----
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_exp(w):
    """Identity below |w| = 1e-10, otherwise AngleAxis(angle, axis).toRotationMatrix() as Eigen writes it."""
    w = np.asarray(w, dtype=F64)
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if theta < 1e-10:
        return np.eye(3)
    a = w / theta
    s, c = math.sin(theta), math.cos(theta)
    sa, ca = s * a, (1.0 - c) * a
    R = np.empty((3, 3))
    tmp = ca[0] * a[1]
    R[0, 1], R[1, 0] = tmp - sa[2], tmp + sa[2]
    tmp = ca[0] * a[2]
    R[0, 2], R[2, 0] = tmp + sa[1], tmp - sa[1]
    tmp = ca[1] * a[2]
    R[1, 2], R[2, 1] = tmp - sa[0], tmp + sa[0]
    for r in range(3):
        R[r, r] = ca[r] * a[r] + c
    return R


def left_jacobian(w):
    w = np.asarray(w, dtype=F64)
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if theta < 1e-10:
        return np.eye(3)
    K = skew(w / theta)
    c1 = (1.0 - math.cos(theta)) / theta
    c2 = (theta - math.sin(theta)) / theta
    KK = np.empty((3, 3))
    for r in range(3):
        for q in range(3):
            KK[r, q] = (K[r, 0] * K[0, q] + K[r, 1] * K[1, q]) + K[r, 2] * K[2, q]
    return (np.eye(3) + c1 * K) + c2 * KK


def left_jacobian_inverse(w):
    w = np.asarray(w, dtype=F64)
    theta = np.linalg.norm(w)
    if theta < 1e-10:
        return np.eye(3)
    K = skew(w / theta)
    c = 1.0 - (1.0 + math.cos(theta)) * theta / (2.0 * math.sin(theta))
    return np.eye(3) - 0.5 * theta * K + c * (K @ K)


def so3_log(R):
    """angle * axis of the rotation (Eigen's AngleAxis(R), taken through the quaternion)."""
    R = np.asarray(R, dtype=F64)
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2.0
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2.0
        q = np.empty(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    n = np.linalg.norm(q[1:])
    if n < 1e-300:
        return np.zeros(3)
    angle = 2.0 * math.atan2(n, abs(q[0]))
    axis = q[1:] / n * (1.0 if q[0] >= 0 else -1.0)
    return np.zeros(3) if angle < 1e-10 else angle * axis


def se3_exp(xi):
    """[v; omega] -> 4 x 4: R = so3Exp(omega), t = leftJacobian(omega) v."""
    xi = np.asarray(xi, dtype=F64)
    v, w = xi[:3], xi[3:]
    T = np.eye(4)
    T[:3, :3] = so3_exp(w)
    J = left_jacobian(w)
    for r in range(3):
        T[r, 3] = (J[r, 0] * v[0] + J[r, 1] * v[1]) + J[r, 2] * v[2]
    return T


def se3_log(T):
    w = so3_log(T[:3, :3])
    return np.concatenate([left_jacobian_inverse(w) @ T[:3, 3], w])


def rigid_mul(A, B):
    """Isometry3d's product, every three-term sum (a0 b0 + a1 b1) + a2 b2."""
    C = np.eye(4)
    for r in range(3):
        for c in range(3):
            C[r, c] = (A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]
        C[r, 3] = ((A[r, 0] * B[0, 3] + A[r, 1] * B[1, 3]) + A[r, 2] * B[2, 3]) + A[r, 3]
    return C


# ---- pieces of the model ----
def robust_weight(residual, kernel, k):
    """computeRobustWeight, vectorised."""
    r = np.abs(np.asarray(residual, dtype=F64))
    with np.errstate(divide="ignore", invalid="ignore"):
        if kernel == HUBER:
            return np.where(r <= k, 1.0, k / r)
        if kernel == TUKEY:
            x = r / k
            t = 1.0 - x * x
            return np.where(r > k, 0.0, t * t)
        if kernel == CAUCHY:
            x = r / k
            return 1.0 / (1.0 + x * x)
    return np.ones_like(r)


def full_hessian(h_upper):
    H = np.zeros((6, 6))
    idx = 0
    for r in range(6):
        for c in range(r, 6):
            H[r, c] = H[c, r] = h_upper[idx]
            idx += 1
    return H


def transform_points(T, x, y, z):
    """float64[n, 3]: ((r0 x + r1 y) + r2 z) + t per row."""
    T = np.asarray(T, dtype=F64)
    x, y, z = (np.asarray(v, dtype=F32).astype(F64) for v in (x, y, z))
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def correspondences(p, tx, ty, tz, max_dist, cells=1 << 23):
    """int64[n]: the target index each transformed source point p (float64[n, 3]) corresponds to, -1 for none."""
    q = p.astype(F32)
    tx, ty, tz = (np.asarray(v, dtype=F32) for v in (tx, ty, tz))
    m = tx.size
    max_d2 = F32(max_dist) * F32(max_dist)
    out = np.full(q.shape[0], -1, dtype=np.int64)
    if m == 0:
        return out
    index = np.arange(m, dtype=np.uint64)
    chunk = max(1, cells // m)
    for a in range(0, q.shape[0], chunk):
        with np.errstate(over="ignore", invalid="ignore"):
            dx = q[a:a + chunk, 0, None] - tx[None, :]
            dy = q[a:a + chunk, 1, None] - ty[None, :]
            dz = q[a:a + chunk, 2, None] - tz[None, :]
            d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        assert d2.dtype == F32
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[None, :]
        best = key.min(axis=1)
        bd2 = (best >> np.uint64(32)).astype(np.uint32).view(F32)
        ok = bd2 <= max_d2
        out[a:a + chunk] = np.where(ok, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    return out


def regularize(cov, eps):
    """float64[n, 3, 3] from float32[n, 3, 3] indexed [row][column]: precomputeRegularizedCovariances.  The lower
    triangle is what Eigen's solver reads.  An exactly diagonal input with equal diagonal gives diag(eps, 1, 1) (ASSUMED)."""
    cov = np.asarray(cov, dtype=F32).reshape(-1, 3, 3)
    n = cov.shape[0]
    out = np.empty((n, 3, 3), dtype=F64)
    A = cov.astype(F64)
    low = np.tril(A)
    A = low + np.transpose(np.tril(A, -1), (0, 2, 1))
    for i in range(n):
        if not np.isfinite(cov[i, 0, 0]):
            out[i] = np.eye(3) * eps
            continue
        a = A[i]
        off = a[1, 0] == 0 and a[2, 0] == 0 and a[2, 1] == 0
        if off and a[0, 0] == a[1, 1] == a[2, 2]:
            v0 = np.array([1.0, 0.0, 0.0])
        else:
            v0 = np.linalg.eigh(a)[1][:, 0]
        f = 1.0 - eps
        out[i] = np.eye(3) - f * np.outer(v0, v0)
    return out


def mat3(A, B):
    """A @ B over leading axes, every three-term sum (a0 b0 + a1 b1) + a2 b2."""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + \
        A[..., :, 2, None] * B[..., None, 2, :]


def terms(method, p, q, kernel=NONE, width=1.0, normals=None, R=None, Cs=None, Ct=None):
    """float64[m, 28]: every correspondence's 21 H (upper triangle, row-major), 6 b and error.  p: transformed source
    points, q: their target points, both float64[m, 3]."""
    tx, ty, tz = p[:, 0], p[:, 1], p[:, 2]
    m = p.shape[0]
    S = np.zeros((m, 28))
    zero, one = np.zeros(m), np.ones(m)
    if method == "icp":
        rx, ry, rz = tx - q[:, 0], ty - q[:, 1], tz - q[:, 2]
        cols = [one, zero, zero, -tz, ty, zero, one, zero, tz, zero, -tx, one, -ty, tx, zero,
                ty * ty + tz * tz, -tx * ty, -tx * tz, tx * tx + tz * tz, -ty * tz, tx * tx + ty * ty,
                rx, ry, rz, ty * rz - tz * ry, tz * rx - tx * rz, tx * ry - ty * rx,
                0.5 * (rx * rx + ry * ry + rz * rz)]
    elif method == "plane":
        nx, ny, nz = normals[:, 0], normals[:, 1], normals[:, 2]
        r = nx * (tx - q[:, 0]) + ny * (ty - q[:, 1]) + nz * (tz - q[:, 2])
        w = robust_weight(np.abs(r), kernel, width)
        j3, j4, j5 = ty * nz - tz * ny, tz * nx - tx * nz, tx * ny - ty * nx
        cols = [w * nx * nx, w * nx * ny, w * nx * nz, w * nx * j3, w * nx * j4, w * nx * j5,
                w * ny * ny, w * ny * nz, w * ny * j3, w * ny * j4, w * ny * j5,
                w * nz * nz, w * nz * j3, w * nz * j4, w * nz * j5,
                w * j3 * j3, w * j3 * j4, w * j3 * j5, w * j4 * j4, w * j4 * j5, w * j5 * j5,
                w * r * nx, w * r * ny, w * r * nz, w * r * j3, w * r * j4, w * r * j5, 0.5 * w * r * r]
    else:
        Rm = np.broadcast_to(np.asarray(R, dtype=F64), (m, 3, 3))
        M = mat3(mat3(Rm, Cs), np.transpose(Rm, (0, 2, 1))) + Ct
        det = M[:, 0, 0] * (M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1]) - \
            M[:, 0, 1] * (M[:, 1, 0] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 0]) + \
            M[:, 0, 2] * (M[:, 1, 0] * M[:, 2, 1] - M[:, 1, 1] * M[:, 2, 0])
        inv_det = 1.0 / det
        w00 = (M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1]) * inv_det
        w01 = (M[:, 0, 2] * M[:, 2, 1] - M[:, 0, 1] * M[:, 2, 2]) * inv_det
        w02 = (M[:, 0, 1] * M[:, 1, 2] - M[:, 0, 2] * M[:, 1, 1]) * inv_det
        w11 = (M[:, 0, 0] * M[:, 2, 2] - M[:, 0, 2] * M[:, 2, 0]) * inv_det
        w12 = (M[:, 0, 2] * M[:, 1, 0] - M[:, 0, 0] * M[:, 1, 2]) * inv_det
        w22 = (M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]) * inv_det
        rx, ry, rz = tx - q[:, 0], ty - q[:, 1], tz - q[:, 2]
        wr0 = w00 * rx + w01 * ry + w02 * rz
        wr1 = w01 * rx + w11 * ry + w12 * rz
        wr2 = w02 * rx + w12 * ry + w22 * rz
        mahal_sq = rx * wr0 + ry * wr1 + rz * wr2
        rw = robust_weight(np.sqrt(np.maximum(mahal_sq, 0.0)), kernel, width)
        w00, w01, w02, w11, w12, w22 = (v * rw for v in (w00, w01, w02, w11, w12, w22))
        wr0, wr1, wr2 = wr0 * rw, wr1 * rw, wr2 * rw
        h03, h04, h05 = -w01 * tz + w02 * ty, w00 * tz - w02 * tx, -w00 * ty + w01 * tx
        h13, h14, h15 = -w11 * tz + w12 * ty, w01 * tz - w12 * tx, -w01 * ty + w11 * tx
        h23, h24, h25 = -w12 * tz + w22 * ty, w02 * tz - w22 * tx, -w02 * ty + w12 * tx
        cols = [w00, w01, w02, h03, h04, h05, w11, w12, h13, h14, h15, w22, h23, h24, h25,
                -(tz * h13 - ty * h23), -(tz * h14 - ty * h24), -(tz * h15 - ty * h25),
                -(-tz * h04 + tx * h24), -(-tz * h05 + tx * h25), -(ty * h05 - tx * h15),
                wr0, wr1, wr2, ty * wr2 - tz * wr1, tz * wr0 - tx * wr2, tx * wr1 - ty * wr0, 0.5 * rw * mahal_sq]
    for a, c in enumerate(cols):
        S[:, a] = c
    return S


def pairwise_sum(v):
    v = list(v)
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else 0.0


def column_sums(S, order):
    if S.shape[0] == 0:
        return np.zeros(S.shape[1])
    if order == "exact":
        return np.array([math.fsum(S[:, a]) for a in range(S.shape[1])])
    if order == "forward":
        return np.array([sum(S[:, a].tolist(), 0.0) for a in range(S.shape[1])])
    if order == "reversed":
        return np.array([sum(S[::-1, a].tolist(), 0.0) for a in range(S.shape[1])])
    assert order == "pairwise"
    return np.array([pairwise_sum(S[:, a].tolist()) for a in range(S.shape[1])])


class Problem:
    """Two clouds and the settings of one registration.  source, target: (x, y, z); normals float32[n_t, 3]; covariances
    float32[n, 3, 3] indexed [row][column]."""

    def __init__(self, method, source, target, target_normals=None, source_cov=None, target_cov=None, **settings):
        unknown = set(settings) - set(DEFAULTS)
        assert not unknown, unknown
        self.method = method
        self.set = dict(DEFAULTS, **settings)
        if isinstance(self.set["robust_kernel"], str):
            self.set["robust_kernel"] = KERNELS[self.set["robust_kernel"]]
        self.s = [np.asarray(v, dtype=F32).reshape(-1) for v in source]
        self.t = [np.asarray(v, dtype=F32).reshape(-1) for v in target]
        self.tq = np.stack(self.t, axis=1).astype(F64)
        self.raw = dict(target_normals=target_normals, source_cov=source_cov, target_cov=target_cov)   # as given
        self.normals = None if target_normals is None else np.asarray(target_normals, dtype=F32).astype(F64)
        eps = self.set["covariance_epsilon"]
        self.Cs = regularize(source_cov, eps) if method == "gicp" else None
        self.Ct = regularize(target_cov, eps) if method == "gicp" else None
        self.n = self.s[0].size

    def linearize(self, T, order="exact"):
        """dict: sums float64[28] (H upper, b, error), abs_sums (the same of |term|), num_inliers, corr int64[n]."""
        T = np.asarray(T, dtype=F64)
        p = transform_points(T, *self.s)
        corr = correspondences(p, *self.t, self.set["max_correspondence_dist"])
        inl = np.flatnonzero(corr >= 0)
        j = corr[inl]
        kern = NONE if self.method == "icp" else self.set["robust_kernel"]
        S = terms(self.method, p[inl], self.tq[j], kern, self.set["robust_kernel_width"],
                  None if self.normals is None else self.normals[j], T[:3, :3],
                  None if self.Cs is None else self.Cs[inl], None if self.Ct is None else self.Ct[j])
        return {"sums": column_sums(S, order), "abs_sums": column_sums(np.abs(S), "exact"), "num_inliers": int(inl.size),
                "corr": corr}


def compute_delta(H, b, lam=LAMBDA):
    return np.linalg.solve(H + lam * np.eye(6), -b)


def converged(delta, prev_error, curr_error, translation_eps, rotation_eps, relative_error_eps):
    """criteria.hpp:40-54 as written: tail<3>() against translation_eps, head<3>() against rotation_eps."""
    dt = math.sqrt(float(delta[3] * delta[3] + delta[4] * delta[4] + delta[5] * delta[5]))
    dr = math.sqrt(float(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]))
    stable = dt < translation_eps and dr < rotation_eps
    rel = abs(prev_error - curr_error) / prev_error if prev_error > 0 else 0.0
    return bool(stable or rel < relative_error_eps)


def covariance_of(H, n_source):
    """inverse(H), or None unless an unpivoted Cholesky finds every pivot above n_source * 2^-52 * max diag(H)."""
    floor = n_source * 2.0 ** -52 * max(0.0, float(np.max(np.diag(H))))
    L = np.zeros((6, 6))
    for j in range(6):
        d = H[j, j] - float(np.dot(L[j, :j], L[j, :j]))
        if not (d > floor) or not np.isfinite(d):
            return None
        L[j, j] = math.sqrt(d)
        for r in range(j + 1, 6):
            L[r, j] = (H[r, j] - float(np.dot(L[r, :j], L[j, :j]))) / L[j, j]
    return np.linalg.inv(H)


class Result:
    def __init__(self, T, fitness, rmse, iterations, converged_, covariance, num_inliers, H):
        self.transform, self.fitness, self.rmse, self.iterations = T, fitness, rmse, iterations
        self.converged, self.covariance, self.num_inliers, self.H = converged_, covariance, num_inliers, H


def failed(T, iterations, num_inliers=0):
    return Result(T, 0.0, math.inf, iterations, False, None, num_inliers, None)


def model_result(T, model, iterations, conv, H, n):
    k = model["num_inliers"] if model else 0
    fitness = k / n if n > 0 else 0.0
    if k > 0:
        rmse = math.sqrt(2.0 * model["sums"][27] / k)
    else:                                                            # makeSuccessResult has no guard: 0 / 0
        rmse = math.nan if conv else math.inf
    Hm = H if H is not None else np.zeros((6, 6))
    return Result(T, fitness, rmse, iterations, conv, covariance_of(Hm, n), k, H)


def align(problem, initial_guess=None, order="forward", trace=None):
    """IterativeSolver<LMOptimizer>::solve (iterative_solver.hpp:96-149) over problem.linearize.  trace: a list that
    receives every iteration's delta."""
    st = problem.set
    T = np.eye(4) if initial_guess is None else np.array(initial_guess, dtype=F64)
    if problem.n == 0 or problem.t[0].size == 0:
        return failed(T, 0)
    prev_error = DBL_MAX
    last_H, last_model = None, None
    for it in range(st["max_iterations"]):
        model = problem.linearize(T, order)
        last_model = model
        if model["num_inliers"] < st["min_correspondences"]:
            return failed(T, it, model["num_inliers"])
        H = full_hessian(model["sums"][:21])
        b = model["sums"][21:27]
        last_H = H
        delta = compute_delta(H, b)
        if trace is not None:
            trace.append(delta)
        new_T = rigid_mul(se3_exp(delta), T)
        err = float(model["sums"][27])
        if converged(delta, prev_error, err, st["translation_eps"], st["rotation_eps"], st["relative_error_eps"]):
            return model_result(new_T, model, it + 1, True, H, problem.n)
        T, prev_error = new_T, err
    return model_result(T, last_model, max(st["max_iterations"], 0), False, last_H, problem.n)


def transform_error(T1, T2):
    """Frobenius norm of T1 * inverse(T2) - I (the reference tests' transformError)."""
    return float(np.linalg.norm(T1 @ np.linalg.inv(T2) - np.eye(4)))
