"""NumPy restatement of nanoPCL's segmentGround and RANSAC segmentPlane / segmentMultiplePlanes, written from the
reference (lib/nanoPCL/include/nanopcl/segmentation/impl/ground_seg_impl.hpp and impl/ransac_plane_impl.hpp; line numbers
below are theirs).  Every fp32 step is explicit: float32 scalars and arrays, one rounding per operation, no contraction.

What the reference leaves open is stated in include/fdm_engine.h and repeated here: the summation order of the
refinement's double sums (taken as a parameter: "forward" as the reference, "reversed", "pairwise") and the sign of the
refined normal (the project's rule: a non-negative dot with the unrefined model's normal, else the first non-zero
component positive)."""
import math

import numpy as np

F = np.float32
INT_MAX = 2 ** 31 - 1
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- RANSAC ----
class XorShift64:  # :29-48
    def __init__(self, seed=42):
        self.state = seed if seed else 1

    def __call__(self):
        s = self.state
        s ^= (s << 13) & M64
        s ^= s >> 7
        s ^= (s << 17) & M64
        self.state = s
        return s

    def rand_index(self, n):
        return self() % n


def draw_triplet(rng, n):  # :265-273: three draws, then the two loops; positions in the index list
    i1, i2, i3 = rng.rand_index(n), rng.rand_index(n), rng.rand_index(n)
    while i2 == i1:
        i2 = rng.rand_index(n)
    while i3 == i1 or i3 == i2:
        i3 = rng.rand_index(n)
    return i1, i2, i3


def triplets(n, count):
    rng = XorShift64(42)
    return [draw_triplet(rng, n) for _ in range(count)]


def adaptive_iterations(ratio, probability):  # :56-71, in double
    if ratio <= 0.0 or ratio >= 1.0:
        return INT_MAX
    w_cubed = ratio * ratio * ratio
    log_prob = math.log(1.0 - probability) if probability < 1.0 else -math.inf
    log_outlier = math.log(1.0 - w_cubed) if w_cubed < 1.0 else -math.inf
    if log_outlier >= 0.0:
        return INT_MAX
    q = log_prob / log_outlier if log_outlier != -math.inf or log_prob != -math.inf else math.nan
    if math.isnan(q) or q >= float(INT_MAX):  # static_cast<int> outside int: saturated (include/fdm_engine.h)
        return INT_MAX
    return max(int(math.ceil(q)), -INT_MAX - 1)


def adaptive_quotient(ratio, probability):
    """log(1 - p) / log(1 - w^3) where computeAdaptiveIterations takes its ceil, else None."""
    if ratio <= 0.0 or ratio >= 1.0 or not probability < 1.0:
        return None
    lo = math.log(1.0 - ratio * ratio * ratio) if ratio * ratio * ratio < 1.0 else -math.inf
    if lo >= 0.0 or lo == -math.inf:
        return None
    return math.log(1.0 - probability) / lo


def sum3(a0, a1, a2):  # the project's three-term order
    return F(a0 + F(a1 + a2))


def plane_from_points(p1, p2, p3):
    """PlaneModel::fromPoints (:196-215): (float32[4], valid)."""
    p1, p2, p3 = (np.asarray(p, dtype=F) for p in (p1, p2, p3))
    with np.errstate(all="ignore"):
        a = [F(p2[k] - p1[k]) for k in range(3)]
        b = [F(p3[k] - p1[k]) for k in range(3)]
        n = [F(F(a[1] * b[2]) - F(a[2] * b[1])),  # Eigen's cross(): (1,2)-(2,1), (2,0)-(0,2), (0,1)-(1,0)
             F(F(a[2] * b[0]) - F(a[0] * b[2])),
             F(F(a[0] * b[1]) - F(a[1] * b[0]))]
        norm = np.sqrt(sum3(F(n[0] * n[0]), F(n[1] * n[1]), F(n[2] * n[2])))
        if norm < F(1e-10):  # :202
            return np.array([0, 0, 0, np.nan], dtype=F), False
        n = [F(c / norm) for c in n]
        d = F(-sum3(F(n[0] * p1[0]), F(n[1] * p1[1]), F(n[2] * p1[2])))
    return np.array([n[0], n[1], n[2], d], dtype=F), bool(np.isfinite(d))  # isValid: ransac_plane.hpp:67


def plane_dist(model, px, py, pz):  # :91 / :114, the scalar expression left to right
    m = np.asarray(model, dtype=F)
    with np.errstate(all="ignore"):
        return np.abs((((m[0] * px).astype(F) + (m[1] * py).astype(F)).astype(F) + (m[2] * pz).astype(F)).astype(F) + m[3])


def collect(x, y, z, indices, model, threshold):  # :102-121
    d = plane_dist(model, x[indices], y[indices], z[indices])
    return indices[d < F(threshold)]


def _ordered_sum(v, order):
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return 0.0
    if order == "forward":
        return float(np.cumsum(v)[-1])
    if order == "reversed":
        return float(np.cumsum(v[::-1])[-1])
    if order == "pairwise":
        return float(_pairwise(v))
    raise ValueError(order)


def _pairwise(v):
    while v.size > 1:
        if v.size & 1:
            v = np.concatenate([v, [0.0]])
        v = v[0::2] + v[1::2]
    return v[0]


def jacobi_smallest(c):
    """Cyclic Jacobi in double on [c00 c01 c02; c01 c11 c12; c02 c12 c22]: the unit eigenvector of the smallest
    eigenvalue."""
    a = [[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(64):
        if not abs(a[0][1]) + abs(a[0][2]) + abs(a[1][2]) > 0.0:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if a[p][q] == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                cs = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * cs
                for k in range(3):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p], a[k][q] = cs * akp - sn * akq, sn * akp + cs * akq
                for k in range(3):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k], a[q][k] = cs * apk - sn * aqk, sn * apk + cs * aqk
                a[p][q] = a[q][p] = 0.0
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p], V[k][q] = cs * vkp - sn * vkq, sn * vkp + cs * vkq
    m = 0
    for k in (1, 2):
        if a[k][k] < a[m][m]:
            m = k
    v = np.array([V[0][m], V[1][m], V[2][m]])
    ln = math.sqrt(V[0][m] * V[0][m] + V[1][m] * V[1][m] + V[2][m] * V[2][m])
    return v / ln if ln > 0.0 else v


def moments(x, y, z, inliers, order="forward"):
    """(centroid[3], c00 c01 c02 c11 c12 c22) of :142-166, in double, summed in `order`."""
    n = inliers.size
    px, py, pz = (v[inliers].astype(np.float64) for v in (x, y, z))
    c = np.array([_ordered_sum(px, order), _ordered_sum(py, order), _ordered_sum(pz, order)]) / float(n)
    dx, dy, dz = px - c[0], py - c[1], pz - c[2]
    mom = [_ordered_sum(v, order) for v in (dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)]
    return c, mom


def refined_model(v, centroid, best_normal):
    """:179-187 with the project's sign rule: the eigenvector cast to float, normalized in fp32, d = -(n . float(c))."""
    n = [F(v[0]), F(v[1]), F(v[2])]
    sq = sum3(F(n[0] * n[0]), F(n[1] * n[1]), F(n[2] * n[2]))
    if sq > F(0):
        norm = np.sqrt(sq)
        n = [F(c / norm) for c in n]
    dot = sum(float(n[k]) * float(best_normal[k]) for k in range(3))  # exact products, summed in double left to right
    flip = dot < 0.0
    if dot == 0.0:
        for k in range(3):
            if n[k] != 0:
                flip = bool(n[k] < 0)
                break
    if flip:
        n = [F(-c) for c in n]
    cf = [F(centroid[k]) for k in range(3)]
    d = F(-sum3(F(n[0] * cf[0]), F(n[1] * cf[1]), F(n[2] * cf[2])))
    return np.array([n[0], n[1], n[2], d], dtype=F)


def refine(x, y, z, inliers, best_model, order="forward", solver="eigh"):  # :134-188
    c, mom = moments(x, y, z, inliers, order)
    if solver == "eigh":
        cov = np.array([[mom[0], mom[1], mom[2]], [mom[1], mom[3], mom[4]], [mom[2], mom[4], mom[5]]])
        v = np.linalg.eigh(cov)[1][:, 0]
    else:
        v = jacobi_smallest(mom)
    return refined_model(v, c, best_model[:3]), mom


def default_result():
    return {"coefficients": np.array([0, 0, 1, 0], dtype=F), "inliers": np.zeros(0, dtype=np.uint32), "fitness": 0.0,
            "iterations": 0, "success": False, "counts": [], "valid": [], "quotients": [], "moments": None,
            "unrefined": np.array([0, 0, 1, 0], dtype=F)}


def ransac_loop(x, y, z, distance_threshold=0.1, max_iterations=1000, probability=0.99, indices=None):
    """The loop of :258-308 alone: what it leaves for finish_plane (the refinement is the only part of segment_plane
    that depends on the summation order or the eigen-solver, so large cases run the loop once and finish it six times)."""
    x, y, z = (np.ascontiguousarray(v, dtype=F).reshape(-1) for v in (x, y, z))
    indices = np.arange(x.size, dtype=np.uint32) if indices is None else np.asarray(indices, dtype=np.uint32).reshape(-1)
    if indices.size and int(indices.max()) >= x.size:
        raise ValueError("an index of the list is not below the point count")
    n = indices.size
    thr = F(distance_threshold)
    loop = {"cloud": (x, y, z), "indices": indices, "threshold": thr, "counts": [], "valid": [], "quotients": [],
            "best_model": np.array([0, 0, 1, 0], dtype=F), "best_count": 0, "loop_iterations": 0}
    if n < 3:  # :247
        return loop
    rng = XorShift64(42)
    best_model, best_count, adaptive, it = loop["best_model"], 0, max_iterations, 0
    lx, ly, lz = x[indices], y[indices], z[indices]
    while it < max_iterations and it < adaptive:  # :258
        it += 1
        i1, i2, i3 = draw_triplet(rng, n)
        pts = [(lx[i], ly[i], lz[i]) for i in (i1, i2, i3)]
        model, valid = plane_from_points(*pts)
        loop["valid"].append(int(valid))
        if not valid:  # :283
            loop["counts"].append(0)
            continue
        count = int(np.count_nonzero(plane_dist(model, lx, ly, lz) < thr))  # :290
        loop["counts"].append(count)
        if count > best_count:  # :296
            best_model, best_count = model, count
            ratio = float(count) / float(n)
            adaptive = adaptive_iterations(ratio, probability)
            q = adaptive_quotient(ratio, probability)
            if q is not None:
                loop["quotients"].append(q)
    loop.update(best_model=best_model, best_count=best_count, loop_iterations=it)
    return loop


def finish_plane(loop, min_inliers=3, refine_model=True, order="forward", solver="eigh"):
    """:310-334 over what ransac_loop left: the result of segment_plane."""
    x, y, z = loop["cloud"]
    indices, thr, n = loop["indices"], loop["threshold"], loop["indices"].size
    res = default_result()
    if n < 3:  # :247
        return res
    res.update(counts=loop["counts"], valid=loop["valid"], quotients=loop["quotients"],
               loop_iterations=loop["loop_iterations"])
    if loop["best_count"] < min_inliers:  # :310
        return res
    best_model = loop["best_model"]
    res["unrefined"] = best_model
    model = best_model
    inl = collect(x, y, z, indices, model, thr)
    if refine_model and inl.size >= 3:  # :321
        refined, mom = refine(x, y, z, inl, best_model, order, solver)
        res["moments"] = mom
        if np.isfinite(refined[3]):  # :323
            model = refined
            inl = collect(x, y, z, indices, model, thr)
    res.update(coefficients=model, inliers=inl, fitness=float(inl.size) / float(n), iterations=loop["loop_iterations"],
               success=bool(np.isfinite(model[3]) and inl.size > 0))
    return res


def segment_plane(x, y, z, distance_threshold=0.1, max_iterations=1000, probability=0.99, min_inliers=3,
                  refine_model=True, indices=None, order="forward", solver="eigh"):
    """:241-334.  Besides the result: counts / valid of every loop pass made (what the engine's replay is fed), the
    quotient log(1 - p) / log(1 - w^3) at every best-update, the refinement's moments, the unrefined model."""
    loop = ransac_loop(x, y, z, distance_threshold, max_iterations, probability, indices)
    return finish_plane(loop, min_inliers, refine_model, order, solver)


def segment_multiple_planes(x, y, z, max_planes=5, min_fitness=0.1, **cfg):  # :366-405
    x = np.ascontiguousarray(x, dtype=F).reshape(-1)
    remaining = np.arange(x.size, dtype=np.uint32)
    out = []
    while len(out) < max_planes and remaining.size >= 3:
        r = segment_plane(x, y, z, indices=remaining, **cfg)
        if not r["success"] or r["fitness"] < min_fitness:
            break
        is_inlier = np.zeros(x.size, dtype=bool)
        is_inlier[r["inliers"]] = True
        remaining = remaining[~is_inlier[remaining]]
        out.append(r)
    return out


def outliers(inliers, total):  # :221-235
    mask = np.ones(total, dtype=bool)
    mask[inliers] = False
    return np.nonzero(mask)[0].astype(np.uint32)


# ---------------------------------------------------------------- ground ----
def cell_coordinates(v, resolution):
    """floor(v / resolution) in fp32 (:33-34): a correctly rounded division; float64 array of the floors."""
    with np.errstate(all="ignore"):
        return np.floor((np.asarray(v, dtype=F) / F(resolution)).astype(F)).astype(np.float64)


def segment_ground(x, y, z, grid_resolution=0.5, cell_percentile=0.2, ground_thickness=0.3, max_ground_height=0.5,
                   min_points_per_cell=2):
    """:68-112: (ground, obstacles), uint32, ascending.  ValueError where the reference is undefined."""
    x, y, z = (np.ascontiguousarray(v, dtype=F).reshape(-1) for v in (x, y, z))
    r, pct = F(grid_resolution), F(cell_percentile)
    if not (np.isfinite(r) and r > 0):
        raise ValueError("resolution must be positive")
    if not pct >= 0:
        raise ValueError("cell_percentile must not be negative or NaN")
    n = x.size
    if n == 0:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    if not (np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(z).all()):
        raise ValueError("a coordinate is not finite")
    gx, gy = cell_coordinates(x, r), cell_coordinates(y, r)
    for g in (gx, gy):
        if not ((g >= -2.0 ** 31) & (g < 2.0 ** 31)).all():
            raise ValueError("a cell does not fit an int32")
    gx, gy = gx.astype(np.int64), gy.astype(np.int64)
    # cells as runs: by cell, inside a cell by z ascending (std::sort of the cell's z values, :52)
    order = np.lexsort((z, gx, gy))
    sx, sy, sz = gx[order], gy[order], z[order]
    head = np.ones(n, dtype=bool)
    head[1:] = (sx[1:] != sx[:-1]) | (sy[1:] != sy[:-1])
    first = np.nonzero(head)[0]
    count = np.diff(np.append(first, n))
    with np.errstate(all="ignore"):
        prod = (pct * (count - 1).astype(F)).astype(F)  # :55: float * float(size_t)
    prod64 = prod.astype(np.float64)
    k = np.where(prod64 < 2.0 ** 32, np.nan_to_num(prod64, nan=2.0 ** 40), 2.0 ** 40)  # size_t(): truncation
    k = np.minimum(np.floor(k).astype(np.int64), count - 1)  # :56
    robust = sz[first + k]  # :57
    obstacle_only = (count < min_points_per_cell) | (robust > F(max_ground_height))  # :46, :60
    with np.errstate(all="ignore"):
        cut = (robust + F(ground_thickness)).astype(F)  # :102, an fp32 sum
    run = np.cumsum(head) - 1
    is_obstacle = np.empty(n, dtype=bool)
    is_obstacle[order] = obstacle_only[run] | (sz > cut[run])  # :100-102
    idx = np.arange(n, dtype=np.uint32)
    return idx[~is_obstacle], idx[is_obstacle]
