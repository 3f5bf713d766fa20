"""nanopcl::filters::voxelGrid (all four modes) and gridMaxZ restated in NumPy, from
lib/nanoPCL/include/nanopcl/filters/impl/voxel_grid_impl.hpp:30-236, grid_max_z_impl.hpp:31-75 and core/voxel.hpp:28-102.

What the GPU filters (fdm_cloud_voxel_grid, fdm_cloud_grid_max_z) are held against, bit for bit.  Every fp32 operation is
a NumPy float32 operation; a run's sums are taken SEQUENTIALLY in the run's order (step k adds the k-th element of every
run that is still open: vectorised across runs, never within one — np.sum would sum pairwise).

order 0: ties in input order (a stable sort); order 1: the order libstdc++'s std::sort leaves the (key, index) pairs in
(scripts/introsort_model.std_sort — slow: keep such clouds under a few thousand points).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import introsort_model as M  # noqa: E402

F32 = np.float32
MODES = ("centroid", "nearest", "any", "center")   # VoxelMode's enum order
OFF = 1 << 20
FLT_MAX = np.finfo(np.float32).max


def size_ok(size):
    """voxel_grid_impl.hpp:31-33 (the C ABI also refuses NaN, which passes both comparisons there)."""
    s = F32(size)
    return bool(s >= F32(0.001)) and bool(s <= F32(100.0))


def _axis(v, inv):
    """One field of voxel::pack: int32(floor(v * inv)) as x86 converts it, clamped, offset."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(v.astype(F32) * inv)
    ok = (f >= F32(-2147483648.0)) & (f < F32(2147483648.0))     # cvttss2si: INT_MIN outside the int range
    i = np.where(ok, f, F32(-2147483648.0)).astype(np.int64)
    return (np.clip(i, -OFF, OFF - 1) + OFF).astype(np.uint64)


def keys_of(x, y, z, size, flat=False):
    """(valid mask, key per point); flat: gridMaxZ's key of (x, y, 0.0f)."""
    x, y, z = (np.asarray(a, dtype=F32) for a in (x, y, z))
    inv = F32(1.0) / F32(size)
    valid = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    kz = np.zeros_like(z) if flat else np.where(valid, z, F32(0))
    kx, ky = np.where(valid, x, F32(0)), np.where(valid, y, F32(0))
    key = (_axis(kz, inv) << np.uint64(42)) | (_axis(ky, inv) << np.uint64(21)) | _axis(kx, inv)
    return valid, key


def unpack(key):
    key = np.asarray(key, dtype=np.uint64)
    m = np.uint64(0x1FFFFF)
    return tuple(((key >> np.uint64(s)) & m).astype(np.int64) - OFF for s in (0, 21, 42))


def sorted_runs(x, y, z, size, order=0, flat=False):
    """(sorted keys, sorted original indices, run starts, run counts) of the valid points."""
    valid, key = keys_of(x, y, z, size, flat)
    vi = np.flatnonzero(valid)
    vk = key[vi]
    if order == 0:
        perm = np.argsort(vk, kind="stable")
    else:
        perm = np.asarray(M.std_sort([int(k) for k in vk]), dtype=np.int64).reshape(-1)
    sk, si = vk[perm], vi[perm]
    if sk.size == 0:
        e = np.zeros(0, dtype=np.int64)
        return sk, si, e, e
    head = np.ones(sk.size, dtype=bool)
    head[1:] = sk[1:] != sk[:-1]
    starts = np.flatnonzero(head)
    counts = np.diff(np.append(starts, sk.size))
    return sk, si, starts, counts


def _run_sums(vals, starts, counts):
    """fp32 sum of every run from 0, in the run's order."""
    acc = np.zeros(starts.size, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(int(counts.max()) if counts.size else 0):
            on = counts > k
            acc[on] = acc[on] + vals[starts[on] + k]
    return acc


def _first_best(score, starts, counts, init, better):
    """Position (in the sorted array) of every run's first entry that beats all before it, starting from `init` with
    the run's first entry."""
    best = np.full(starts.size, init, dtype=F32)
    at = starts.copy()
    for k in range(int(counts.max()) if counts.size else 0):
        on = np.flatnonzero(counts > k)
        j = starts[on] + k
        win = better(score[j], best[on])
        best[on[win]] = score[j[win]]
        at[on[win]] = j[win]
    return at


def _take(ch, i):
    return {k: (v[i].copy() if v is not None else None) for k, v in ch.items()}


def _channels(x, y, z, intensity, rgb, normals, cov):
    n = np.asarray(x).size
    ch = {"x": np.asarray(x, dtype=F32), "y": np.asarray(y, dtype=F32), "z": np.asarray(z, dtype=F32),
          "intensity": None if intensity is None else np.asarray(intensity, dtype=F32),
          "rgb": None if rgb is None else np.asarray(rgb, dtype=np.uint32),
          "nx": None, "ny": None, "nz": None,
          "cov9": None if cov is None else np.asarray(cov, dtype=F32).reshape(n, 9)}
    if normals is not None:
        ch["nx"], ch["ny"], ch["nz"] = (np.asarray(a, dtype=F32) for a in normals)
    return ch


def voxel_grid(x, y, z, size, mode="centroid", intensity=None, rgb=None, normals=None, cov=None, order=0):
    """dict of the output channels (absent ones None) and "idx" (uint32: the point copied, or the run's rep)."""
    if not size_ok(size):
        raise ValueError("voxel_size must be in [0.001, 100]")
    assert mode in MODES
    ch = _channels(x, y, z, intensity, rgb, normals, cov)
    sk, si, starts, counts = sorted_runs(ch["x"], ch["y"], ch["z"], size, order)
    if mode == "any":
        s, c = starts.astype(object), counts.astype(object)        # size_t arithmetic: no wrap below 2^64 here
        pick = np.array([int(a + (b * 7 + a * 13) % b) for a, b in zip(s, c)], dtype=np.int64)
        w = si[pick]
        return dict(_take(ch, w), idx=w.astype(np.uint32))
    size32 = F32(size)
    ix, iy, iz = unpack(sk[starts])
    cx, cy, cz = ((i.astype(F32) + F32(0.5)) * size32 for i in (ix, iy, iz))     # voxel::toCenter
    if mode == "nearest":
        run = np.repeat(np.arange(starts.size), counts)
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy, dz = ch["x"][si] - cx[run], ch["y"][si] - cy[run], ch["z"][si] - cz[run]
            d2 = (dx * dx + dz * dz) + (dy * dy + F32(0))            # Eigen's 4-float packet reduction (ASSUMED)
        w = si[_first_best(d2.astype(F32), starts, counts, FLT_MAX, lambda a, b: a < b)]
        return dict(_take(ch, w), idx=w.astype(np.uint32))
    rep = si[starts]
    cnt = counts.astype(F32)
    out = {k: None for k in ch}
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if mode == "centroid":
            for k in ("x", "y", "z"):
                out[k] = _run_sums(ch[k][si], starts, counts) / cnt
        else:
            out["x"], out["y"], out["z"] = cx, cy, cz
        if ch["intensity"] is not None:
            out["intensity"] = _run_sums(ch["intensity"][si], starts, counts) / cnt
        if ch["rgb"] is not None:
            c = ch["rgb"][si]
            parts = [(_run_sums(((c >> np.uint32(s)) & np.uint32(255)).astype(F32), starts, counts) / cnt)
                     .astype(np.int32).astype(np.uint32) & np.uint32(255) for s in (16, 8, 0)]
            out["rgb"] = (parts[0] << np.uint32(16)) | (parts[1] << np.uint32(8)) | parts[2]
        if ch["nx"] is not None:
            sx, sy, sz = (_run_sums(ch[k][si], starts, counts) for k in ("nx", "ny", "nz"))
            norm = np.sqrt((sx * sx + sy * sy) + sz * sz)
            ok = norm > F32(1e-6)
            safe = np.where(ok, norm, F32(1))
            out["nx"] = np.where(ok, sx / safe, F32(0)).astype(F32)
            out["ny"] = np.where(ok, sy / safe, F32(0)).astype(F32)
            out["nz"] = np.where(ok, sz / safe, F32(1)).astype(F32)
    if ch["cov9"] is not None:
        out["cov9"] = ch["cov9"][rep].copy()
    out["idx"] = rep.astype(np.uint32)
    return out


def grid_max_z(x, y, z, size, intensity=None, rgb=None, normals=None, cov=None, order=0):
    """gridMaxZ: per (x, y) cell the first strictly greatest z in the run's order, every channel that point's."""
    if not size_ok(size):
        raise ValueError("grid_size must be in [0.001, 100]")
    ch = _channels(x, y, z, intensity, rgb, normals, cov)
    sk, si, starts, counts = sorted_runs(ch["x"], ch["y"], ch["z"], size, order, flat=True)
    zs = ch["z"][si]
    best = zs[starts] if starts.size else np.zeros(0, dtype=F32)
    at = starts.copy()
    for k in range(1, int(counts.max()) if counts.size else 0):
        on = np.flatnonzero(counts > k)
        j = starts[on] + k
        win = zs[j] > best[on]
        best[on[win]] = zs[j[win]]
        at[on[win]] = j[win]
    w = si[at]
    return dict(_take(ch, w), idx=w.astype(np.uint32))
