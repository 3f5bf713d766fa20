"""Clouds for the normal-estimation tests (tests/test_normal_restate.py proves on the CPU which path of the search each
is meant to reach, tests/test_normals_gpu.py runs them on the device), and the restatement's answers to them, computed
once per process.  Test data, not product."""
import functools

import numpy as np

import dem_restate as DR
import normal_restate as NR

F32 = np.float32
SHELLS = 4                                                           # kKnnShells (fdm_knn.hpp)


# ---- the reference's own test clouds (lib/nanoPCL/tests/test_geometry.cpp:24-76) ----
def plane_xy(n=10, z=0.0):
    i, j = np.divmod(np.arange(n * n), n)
    return i.astype(F32), j.astype(F32), np.full(n * n, z, dtype=F32)


def plane_xz(n=10, y=0.0):
    i, j = np.divmod(np.arange(n * n), n)
    return i.astype(F32), np.full(n * n, y, dtype=F32), j.astype(F32)


def plane_tilted(n=10):
    i, j = np.divmod(np.arange(n * n), n)
    x, y = i.astype(F32), j.astype(F32)
    return x, y, F32(0.5) * x + F32(0.3) * y


def sparse():
    return np.array([0, 1], dtype=F32), np.zeros(2, dtype=F32), np.zeros(2, dtype=F32)


def collinear():
    return np.arange(10, dtype=F32), np.zeros(10, dtype=F32), np.zeros(10, dtype=F32)


# ---- clouds of this project's tests ----
def surface(n, seed, span=8.0, shift=(0.0, 0.0, 0.0)):
    """n points of arbitrary fp32 coordinates on a gently rolling surface over [0, span)^2, then shifted."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, span, n)
    y = rng.uniform(0.0, span, n)
    z = 0.3 * np.sin(x * (6.0 / span)) + 0.2 * np.cos(y * (5.0 / span)) + rng.normal(0.0, 0.01, n)
    return tuple((v + s).astype(F32) for v, s in zip((x, y, z), shift))


def cloud(name):
    if name == "surface":                                            # the bucket edges, the forms, host and device
        return surface(4096, 31)
    if name.startswith("n"):                                         # k against n; the block and wave sizes
        n = int(name[1:])
        return surface(n, 2000 + n, span=2.0)
    if name == "isolated":                                           # a dense patch and six points far from it: the queue
        x, y, z = surface(2000, 32, span=2.0)
        far = np.array([[60, 55, 1], [-50, 40, 0], [45, -62, 2], [-58, -47, 0], [70, 3, 1], [2, 66, 0]], dtype=F32)
        at = np.array([5, 400, 801, 1203, 1604, 1999])
        x[at], y[at], z[at] = far[:, 0], far[:, 1], far[:, 2]
        return x, y, z
    if name == "small_grid":                                         # at most 5 x 5 columns: every lane sees the whole cloud
        return surface(60, 33, span=3.0)
    if name == "identical":
        return tuple(np.full(100, v, dtype=F32) for v in (1.5, -2.25, 0.75))
    if name == "collinear":
        return collinear()
    if name == "duplicates":                                         # copies of one point at lower and higher indices
        x, y, z = surface(300, 34, span=2.0)
        for c in (x, y, z):
            c[[3, 77, 150, 151, 290]] = c[150]
        return x, y, z
    if name in ("xy5", "xy10"):
        return plane_xy(int(name[2:]))
    if name in ("xz5", "xz10"):
        return plane_xz(int(name[2:]))
    if name in ("tilted5", "tilted10"):
        return plane_tilted(int(name[6:]))
    if name == "utm":                                                # the same kind of surface at UTM-sized coordinates
        return surface(4096, 35, span=64.0, shift=(5.0e5, 4.9e5, 120.0))
    if name == "large":
        return surface(200_000, 36, span=120.0, shift=(5.0e5, 4.9e5, 120.0))
    raise KeyError(name)


LARGE_QUERIES = 512


def rows_of(name):
    """The queries a case is compared at: every point, but a seeded sample of the large cloud."""
    if name == "large":
        return np.sort(np.random.default_rng(37).permutation(200_000)[:LARGE_QUERIES])
    return None


@functools.lru_cache(maxsize=None)
def _table(name):
    """The 64 (or n) nearest of every compared query by (d2, index): a smaller k's neighbours are its first k."""
    x, y, z = cloud(name)
    rows = rows_of(name)
    return NR.neighbours(x, y, z, min(NR.MAX_K, x.size), np.arange(x.size) if rows is None else rows)


@functools.lru_cache(maxsize=None)
def restated(name, k, viewpoint=(0.0, 0.0, 0.0)):
    """((x, y, z), rows or None, normals, cov, invalid) of the restatement, read-only."""
    x, y, z = cloud(name)
    k_eff = NR.effective_k(x.size, k)
    assert k_eff <= NR.MAX_K
    idx = _table(name)[:, :k_eff] if k_eff >= NR.MIN_NEIGHBORS else None
    out = NR.estimate(x, y, z, k, viewpoint, rows=rows_of(name), idx=idx)
    for a in (x, y, z) + out:
        a.setflags(write=False)
    return (x, y, z), rows_of(name), out[0], out[1], out[2]


def grid_of(name, k):
    """(h, gx, gy, cx, cy): the search grid the engine builds for the cloud and every point's column in it."""
    x, y, _ = cloud(name)
    k_eff = NR.effective_k(x.size, k)
    h, gx, gy = DR.sor_grid(x.min(), y.min(), x.max(), y.max(), x.size, k_eff)
    return h, gx, gy, DR.knn_columns(x, x.min(), h, gx), DR.knn_columns(y, y.min(), h, gy)


def must_queue(name, k):
    """How many points of the cloud cannot be settled by the ring search and so have to take the queue: after ring s a
    lane is settled only if its k-th distance is below (s + margin) h with margin <= 1/2, or if the rings have covered
    the grid — so a point whose k-th neighbour is further than (SHELLS + 1/2) h, in a grid that goes on beyond ring
    SHELLS around its column, is queued.  (Sufficient, not necessary: the engine may queue more.)"""
    x, y, z = cloud(name)
    k_eff = NR.effective_k(x.size, k)
    h, gx, gy, cx, cy = grid_of(name, k)
    far = np.flatnonzero(np.maximum(np.abs(x), np.abs(y)) > 30)      # (only the few far points are worth the brute force)
    kth = NR.kth_distance(x, y, z, k_eff, far)
    covered = (cx[far] - SHELLS <= 0) & (cx[far] + SHELLS >= gx - 1) & (cy[far] - SHELLS <= 0) & (cy[far] + SHELLS >= gy - 1)
    return int(((kth > (SHELLS + 0.5) * float(h)) & ~covered).sum())
