"""nanopcl::filters::radiusOutlierRemoval, the crop family and removeInvalid restated in NumPy from what the reference
does (filters/impl/outlier_removal_impl.hpp:21-77, filters/impl/crop_impl.hpp, filters/core.hpp:95-109).

Radius outlier removal twice: at the reference's table and chain level — tests/cluster_restate.py's VoxelHash, built over
the cloud and asked for radius() per point, idx != i counted — and from the relation alone, by testing pairs.  fp32
throughout, dist_sq in the three-term order the project fixes.

The crop predicates comparison by comparison, in fp32.  cropAngle's four constants come from libm's cosf / sinf through
ctypes — what a build of the reference calls — not from np.cos, whose float32 kernels may differ by an ulp."""
import ctypes
import ctypes.util

import numpy as np

import cluster_restate as CR

F = np.float32


# ---- radius outlier removal ----
def radius_counts_reference(pts, radius):
    """count[i] as the reference's loop finds it: VoxelHash(radius).build(cloud), radius(point i, radius), idx != i."""
    n = pts.shape[0]
    counts = np.zeros(n, dtype=np.uint32)
    if n == 0:
        return counts
    search = CR.VoxelHash(radius)
    search.build(pts)
    for i in range(n):
        nb = search.radius(pts[i], radius)
        counts[i] = int((nb != i).sum())
    return counts


def radius_counts_brute(pts, radius):
    """count[i] from the relation alone: the j != i whose voxels differ from i's by at most `range` on every axis and
    whose dist_sq <= r_sq."""
    n = pts.shape[0]
    counts = np.zeros(n, dtype=np.int64)
    if n < 2:
        return counts.astype(np.uint32)
    inv, r_sq, rng = CR.relation_constants(radius)
    vox = CR.voxels(pts, inv)
    for i, j, _ in CR.near_pairs(pts, radius, rng):
        ok = (np.abs(vox[i] - vox[j]) <= rng).all(axis=1) & (CR.dist_sq(pts[i], pts[j]) <= r_sq)
        np.add.at(counts, i[ok], 1)
        np.add.at(counts, j[ok], 1)
    return counts.astype(np.uint32)


def candidate_tests(pts, radius):
    """The work bound's measure: per point the OTHER points in the (2 range + 1)^3 voxels around its own, summed."""
    n = pts.shape[0]
    if n == 0:
        return 0
    inv, _, rng = CR.relation_constants(radius)
    vox = CR.voxels(pts, inv)
    uniq, inverse, occupancy = np.unique(vox, axis=0, return_inverse=True, return_counts=True)
    table = {tuple(v): int(c) for v, c in zip(uniq.tolist(), occupancy)}
    total = 0
    span = range(-rng, rng + 1)
    for v, c in table.items():
        near = sum(table.get((v[0] + dx, v[1] + dy, v[2] + dz), 0) for dx in span for dy in span for dz in span)
        total += c * (near - 1)
    return total


def admitted(pts, radius):
    """What fdm_cloud_radius_outlier_removal accepts: finite coordinates, voxels inside -2^20 + range .. 2^20 - 1 - range."""
    if not np.isfinite(pts).all():
        return False
    inv, _, rng = CR.relation_constants(radius)
    f = np.floor(pts * F(inv))
    return bool(pts.shape[0] == 0 or (f.min() >= CR.COORD_MIN + rng and f.max() <= CR.COORD_MAX - rng))


# ---- the predicate filters ----
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _name in ("cosf", "sinf"):
    getattr(_libm, _name).restype = ctypes.c_float
    getattr(_libm, _name).argtypes = [ctypes.c_float]


def angle_constants(min_angle, max_angle):
    """crop_impl.hpp:188-195 in fp32: (cos_min, sin_min, cos_max, sin_max, wrap, range, use_and)."""
    lo, hi = F(min_angle), F(max_angle)
    cs = [F(_libm.cosf(float(lo))), F(_libm.sinf(float(lo))), F(_libm.cosf(float(hi))), F(_libm.sinf(float(hi)))]
    wrap = bool(lo > hi)
    pi = F(np.pi)
    span = (F(2.0) * pi - (lo - hi)) if wrap else (hi - lo)
    return (*cs, wrap, F(span), bool(F(span) < pi))


def _xyz(x, y, z):
    return (np.asarray(v, dtype=F) for v in (x, y, z))


def crop_box(x, y, z, lo, hi, mode="inside"):
    x, y, z = _xyz(x, y, z)
    lo, hi = np.asarray(lo, dtype=F), np.asarray(hi, dtype=F)
    with np.errstate(all="ignore"):
        if mode == "inside":
            return (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
        return (x < lo[0]) | (x > hi[0]) | (y < lo[1]) | (y > hi[1]) | (z < lo[2]) | (z > hi[2])


def crop_range(x, y, z, min_range, max_range, mode="inside"):
    x, y, z = _xyz(x, y, z)
    with np.errstate(all="ignore"):
        min_sq, max_sq = F(min_range) * F(min_range), F(max_range) * F(max_range)
        d2 = x * x + (y * y + z * z)
        return ((d2 >= min_sq) & (d2 <= max_sq)) if mode == "inside" else ((d2 < min_sq) | (d2 > max_sq))


def crop_axis(v, lo, hi, mode="inside"):
    v, lo, hi = np.asarray(v, dtype=F), F(lo), F(hi)
    with np.errstate(all="ignore"):
        return ((v >= lo) & (v <= hi)) if mode == "inside" else ((v < lo) | (v > hi))


def crop_angle(x, y, z, min_angle, max_angle, mode="inside"):
    x, y, z = _xyz(x, y, z)
    cos_min, sin_min, cos_max, sin_max, _, _, use_and = angle_constants(min_angle, max_angle)
    eps = F(1e-5)
    with np.errstate(all="ignore"):
        c_min = cos_min * y - sin_min * x
        c_max = cos_max * y - sin_max * x
        a, b = c_min >= -eps, c_max <= eps
        in_range = (a & b) if use_and else (a | b)
    return in_range == (mode == "inside")


def remove_invalid(x, y, z):
    x, y, z = _xyz(x, y, z)
    return np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
