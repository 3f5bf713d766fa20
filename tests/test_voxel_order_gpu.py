"""Option voxel_any_order = 1: VoxelMode::ANY picks the point a g++ build of the reference picks (the order libstdc++'s
std::sort leaves inside a voxel, fdm_introsort.hpp), engine against the ORACLE's std::sort variant, bit for bit.

Every input also shows that the option matters: the stable order (option 0, the oracle's default) picks differently.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from helpers import assert_layers_bit_identical, same_geometry
from test_batch_gpu import DeviceBatch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import introsort_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def check_voxel_any(gpu, R, x, y, z, size, differs=True):
    eng = gpu.Engine(4.0, 4.0, 0.5)
    eng.set_option("voxel_any_order", 1)
    got = eng.voxel_any(x, y, z, size)
    want = R.voxel_any(x, y, z, size, stable=False)
    assert got.size == want.size, (got.size, want.size)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} picks differ"
    stable = R.voxel_any(x, y, z, size, stable=True)
    if differs:
        assert not np.array_equal(stable, want), "input without teeth: std::sort and the stable order agree"
    eng.set_option("voxel_any_order", 0)
    assert np.array_equal(eng.voxel_any(x, y, z, size), stable)
    eng.close()


def tied_cloud(rng, n, cells, span=4.0):
    """n points in about `cells` voxels of 0.25 m: every voxel holds several."""
    c = rng.integers(0, cells, n)
    side = max(1, int(round(cells ** (1 / 3))))
    x = (c % side) * 0.25 + rng.uniform(0.01, 0.24, n)
    y = ((c // side) % side) * 0.25 + rng.uniform(0.01, 0.24, n)
    z = (c // (side * side)) * 0.25 + rng.uniform(0.01, 0.24, n)
    return x.astype(F32) - F32(span / 2), y.astype(F32) - F32(span / 2), z.astype(F32)


@pytest.mark.parametrize("n", [1, 2, 16, 17, 31, 33, 1000, 28800, 300000, 2100000])
def test_voxel_any_sizes(gpu, R, n):
    rng = np.random.default_rng(n)
    x, y, z = tied_cloud(rng, n, max(1, n // 8))
    check_voxel_any(gpu, R, x, y, z, 0.25, differs=n > 16)   # (up to 16 points std::sort is an insertion sort: stable)


@pytest.mark.parametrize("shape", ["one_voxel", "two_alternating", "sorted", "reversed", "organ_pipe"])
@pytest.mark.parametrize("n", [33, 5000, 70000])
def test_voxel_any_key_orders(gpu, R, shape, n):
    rng = np.random.default_rng(len(shape) * 100 + n)
    if shape == "one_voxel":
        v = np.zeros(n)
    elif shape == "two_alternating":
        v = (np.arange(n) % 2).astype(float)
    else:
        v = np.sort(rng.integers(0, max(2, n // 10), n)).astype(float)
        if shape == "reversed":
            v = v[::-1].copy()
        elif shape == "organ_pipe":
            v = np.minimum(np.arange(n), n - 1 - np.arange(n)) // 5
    x = (v * 0.25 + rng.uniform(0.01, 0.24, n)).astype(F32)
    y = rng.uniform(0.01, 0.24, n).astype(F32)
    z = rng.uniform(0.01, 0.24, n).astype(F32)
    check_voxel_any(gpu, R, x, y, z, 0.25)


def test_voxel_any_non_finite_and_far_off(gpu, R):
    rng = np.random.default_rng(5)
    n = 60000
    x, y, z = tied_cloud(rng, n, 4000)
    bad = rng.random(n) < 0.1
    x[bad & (rng.random(n) < 0.5)] = np.nan
    y[bad & (rng.random(n) < 0.5)] = np.inf
    z[bad] = -np.inf
    check_voxel_any(gpu, R, x, y, z, 0.25)
    # UTM-like coordinates: voxel indices beyond the key's clamp range
    check_voxel_any(gpu, R, x + F32(5.3e5), y + F32(5.3e6), z, 0.25)


@pytest.mark.parametrize("workload", ["vlp16", "rgbd", "lidar128"])
def test_voxel_any_sensor_scans(gpu, R, workload):
    """Scans of the synthetic sensors in their own point order (firing order, image rows), whose keys arrive in runs."""
    wl = getattr(gpu.synth, workload)(n_scans=1)
    s = wl.scan(0)
    check_voxel_any(gpu, R, s["x"], s["y"], s["z"], wl.resolution)


@pytest.mark.parametrize("n", [2000, 5000, 40000])
def test_depth_limit_heap_fallback(gpu, R, n):
    """A median-of-3 killer: the restatement proves that a range reaches the depth limit with ties in it (2000: inside
    one workgroup's LDS; 5000, 40000: a range too large for it)."""
    keys = M.median3_killer(n)
    rep = {}
    M.std_sort(keys, rep)
    assert any(ties for _, _, ties in rep["heap_ranges"]), rep["heap_ranges"]
    k = np.asarray(keys, dtype=np.float64)
    rng = np.random.default_rng(n)
    x = (k * 0.25 + 0.125).astype(F32) - F32(600.0)
    y = rng.uniform(0.01, 0.24, n).astype(F32)
    z = np.full(n, 0.1, dtype=F32)
    check_voxel_any(gpu, R, x, y, z, 0.25)


# ------------------------------------------------------------------------------------------------- integrate ----
SENSOR_Z = 1.1


def cfg_fill(c, mode=0):
    c.mode = mode
    c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 4.0, 0.2, 14.0
    c.raycast_enabled = 1
    c.rc_log_odds_ghost, c.rc_clear_threshold, c.rc_height_conflict_threshold = 0.9, -0.5, 0.02
    return c


def scan(rng, n, rgb=False, spread=11.0):
    x = rng.uniform(-spread, spread, n).astype(F32)
    y = rng.uniform(-spread, spread, n).astype(F32)
    z = (rng.uniform(-0.6, 0.5, n) - SENSOR_Z).astype(F32)
    s = {"x": x, "y": y, "z": z, "intensity": rng.uniform(0, 1, n).astype(F32)}
    if rgb:
        s["rgb"] = rng.integers(0, 1 << 24, n).astype(np.uint32)
        del s["intensity"]
    return s


def plant_ghosts(objs, seed):
    r = np.random.default_rng(seed)
    e = objs[0].layer("elevation").copy()
    rows, cols = e.shape
    for _ in range(6):
        r0, c0 = int(r.integers(4, rows - 12)), int(r.integers(4, cols - 12))
        e[r0:r0 + 8, c0:c0 + 8] = F32(1.25)
    for o in objs:
        o.set_layer("elevation", e)


def kw_of(s):
    return {k: s[k] for k in ("intensity", "rgb") if s.get(k) is not None}


class Stream:
    """Engine with the option on, the oracle with std::sort's order, and a stable oracle that must end elsewhere."""

    def __init__(self, gpu, R, size=24.0, res=0.1, position=(0.0, 0.0), fill=cfg_fill, Tbs=None, **opts):
        self.gpu = gpu
        self.eng = gpu.Engine(size, size, res, fill(gpu.capi.default_config()), position=position)
        self.ref = R.RefEngine(size, size, res, fill(R.default_config()), position=position)
        self.stb = R.RefEngine(size, size, res, fill(R.default_config()), position=position)
        self.eng.set_option("voxel_any_order", 1)
        self.ref.set_voxel_stable(False)
        for k, v in opts.items():
            self.eng.set_option(k, v)
        if Tbs is None:
            Tbs = np.eye(4)
            Tbs[2, 3] = SENSOR_Z
        self.Tbs = Tbs
        self.keep = []

    def oracles(self, s, T):
        st = self.ref.integrate(s["x"], s["y"], s["z"], self.Tbs, T, **kw_of(s))
        self.stb.integrate(s["x"], s["y"], s["z"], self.Tbs, T, **kw_of(s))
        return st

    def run(self, scans, poses, how):
        stats = [self.oracles(s, T) for s, T in zip(scans, poses)]
        e = self.eng
        if how == "sync":
            for s, T, st in zip(scans, poses, stats):
                assert e.integrate(s["x"], s["y"], s["z"], self.Tbs, T, **kw_of(s)) == st
        elif how == "points4":
            for s, T, st in zip(scans, poses, stats):
                xyz1 = np.stack([s["x"], s["y"], s["z"], np.ones_like(s["x"])], axis=1).astype(F32)
                assert e.integrate_points4(xyz1, self.Tbs, T, **kw_of(s)) == st
        elif how == "async":
            for s, T in zip(scans, poses):
                e.integrate_async(s["x"], s["y"], s["z"], self.Tbs, T, **kw_of(s))
        elif how == "device":
            import torch
            for s, T in zip(scans, poses):
                d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in s.items() if v is not None}
                self.keep.append(d)
                e.integrate_device(d["x"], d["y"], d["z"], self.Tbs, T, **{k: d[k] for k in kw_of(s)})
        elif how == "device_batch":
            b = DeviceBatch(self.gpu, scans, self.Tbs, poses)
            self.keep.append(b)
            assert e.integrate_device_batch(b.arr) == 0
        elif how == "host_batch":
            arr = (self.gpu.capi.FdmDeviceScan * len(scans))()
            for i, (s, T) in enumerate(zip(scans, poses)):
                d = arr[i]
                d.n = int(s["x"].size)
                for c in ("x", "y", "z", "intensity", "rgb"):
                    if s.get(c) is not None:
                        a = np.ascontiguousarray(s[c])
                        self.keep.append(a)
                        setattr(d, c, a.ctypes.data)
                    else:
                        setattr(d, c, None)
                d.sigma_z2 = None
                d.T_base_sensor = (ctypes.c_double * 16)(*np.asarray(self.Tbs, float).T.reshape(16))
                d.T_world_base = (ctypes.c_double * 16)(*np.asarray(T, float).T.reshape(16))
            self.keep.append(arr)
            e.integrate_host_batch(arr)
        else:
            raise AssertionError(how)
        return stats[-1]

    def compare(self, what, stats=None):
        e = self.eng
        e.sync()
        self.keep.clear()
        try:
            assert_layers_bit_identical(e, self.ref)
        except AssertionError as err:
            raise AssertionError(f"{what}: {err}") from None
        assert same_geometry(e.geometry(), self.ref.geometry()), what
        if stats is not None:
            assert e.last_stats() == stats, (what, e.last_stats(), stats)

    def stable_differs(self):
        """The stable oracle ends with another map for the same scans: the option has teeth."""
        for name in ("raycasting", "_visibility_logodds", "ghost_removal", "elevation"):
            a, b = self.ref.layer(name), self.stb.layer(name)
            if not np.array_equal(np.isnan(a), np.isnan(b)) or not np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]):
                return True
        return False


def poses_walk(rng, k, pose):
    out = []
    for _ in range(k):
        pose[0] += float(rng.uniform(-0.25, 0.35))
        pose[1] += float(rng.uniform(-0.2, 0.2))
        T = np.eye(4)
        T[0, 3], T[1, 3] = pose
        out.append(T)
    return out


@pytest.mark.parametrize("how", ["sync", "async", "device", "points4", "device_batch", "host_batch"])
def test_integrate_vlp16_stream_local_moves(gpu, R, how):
    S = Stream(gpu, R)
    rng = np.random.default_rng(31 + len(how))
    pose = [0.0, 0.0]
    for g in range(4):
        if g:
            plant_ghosts([S.eng, S.ref, S.stb], 90 + g)
        scans = [scan(rng, 28800) for _ in range(3)]
        st = S.run(scans, poses_walk(rng, 3, pose), how)
        S.compare(f"{how}, group {g}", st)
    assert S.stable_differs()


def synth_fill(wl, **extra):
    def fill(c):
        wl.apply_to(c)
        c.raycast_enabled = 1
        for k, v in extra.items():
            setattr(c, k, v)
        return c
    return fill


def test_integrate_rgbd_p2_colour(gpu, R):
    """The RGB-D workload as it ships: P² estimator, RGB-D sensor model, colour, camera key order, LOCAL moves."""
    wl = gpu.synth.rgbd(n_scans=3)
    assert wl.estimation_type == 1 and wl.sensor_type == 2
    S = Stream(gpu, R, size=wl.width, res=wl.resolution, fill=synth_fill(wl), Tbs=wl.T_base_sensor)
    for k in range(3):
        if k:
            plant_ghosts([S.eng, S.ref, S.stb], 5 + k)
        S.compare(f"rgbd scan {k}", S.run([wl.scan(k)], [wl.pose(k)], "sync"))
    assert "color" in S.eng.layers()
    assert S.stable_differs()


def test_integrate_lidar128_full_size(gpu, R):
    """Two 2.1 M-point LiDAR scans in firing (azimuth) order: the key order the level passes see on a real sensor."""
    wl = gpu.synth.lidar128(n_scans=2)
    assert wl.n_points == 2097152
    S = Stream(gpu, R, size=wl.width, res=wl.resolution, fill=synth_fill(wl), Tbs=wl.T_base_sensor)
    S.compare("lidar128 scan 0", S.run([wl.scan(0)], [wl.pose(0)], "sync"))
    plant_ghosts([S.eng, S.ref, S.stb], 9)
    S.compare("lidar128 scan 1", S.run([wl.scan(1)], [wl.pose(1)], "sync"))
    assert S.stable_differs()


def test_integrate_global_map_sensor_outside(gpu, R):
    """A GLOBAL map (it does not follow the sensor) and scans from a sensor outside it: the stage does not run there
    (raycasting.cpp:217-220), so the frame layer appears only once the sensor has been inside and then keeps its values
    while it is outside."""
    S = Stream(gpu, R, size=16.0, res=0.1, position=(3.0, -2.0), fill=lambda c: cfg_fill(c, mode=1))
    rng = np.random.default_rng(8)
    outside = (20.0, 0.0)
    before = None
    for k, pos in enumerate([outside, (1.0, 0.0), (2.0, -1.0), outside, (3.0, -2.5)]):
        T = np.eye(4)
        T[0, 3], T[1, 3] = pos
        s = scan(rng, 40000, spread=9.0)
        st = S.oracles(s, T)
        assert S.eng.integrate(s["x"], s["y"], s["z"], S.Tbs, T, **kw_of(s)) == st
        S.compare(f"global scan {k}", st)
        g = S.eng.geometry()
        assert (g.position_x, g.position_y) == (3.0, -2.0), "a GLOBAL map does not move"
        if k == 0:
            assert not S.eng.exists("raycasting") and not S.ref.exists("raycasting")
        if k == 1:
            assert S.eng.exists("raycasting")
            plant_ghosts([S.eng, S.ref, S.stb], 3)
        if k == 3:
            assert np.array_equal(S.eng.layer("raycasting"), before, equal_nan=True)
        before = S.eng.layer("raycasting").copy() if S.eng.exists("raycasting") else None
    assert S.stable_differs()


def test_integrate_ray_overlap_mixed_sizes(gpu, R):
    S = Stream(gpu, R, ray_overlap=1, ray_large_min=20000)
    rng = np.random.default_rng(12)
    pose = [0.0, 0.0]
    for g, sizes in enumerate([[3000, 25000, 60000], [60000, 60000, 3000], [25000, 70000, 70000, 4000]]):
        if g:
            plant_ghosts([S.eng, S.ref, S.stb], 40 + g)
        scans = [scan(rng, n) for n in sizes]
        S.compare(f"overlap group {g}", S.run(scans, poses_walk(rng, len(sizes), pose), "async"))
    assert S.stable_differs()


def test_integrate_option_toggled_mid_stream(gpu, R):
    S = Stream(gpu, R)
    rng = np.random.default_rng(21)
    pose = [0.0, 0.0]
    for g, on in enumerate([1, 0, 1]):
        S.eng.set_option("voxel_any_order", on)
        S.ref.set_voxel_stable(not on)
        if g:
            plant_ghosts([S.eng, S.ref, S.stb], 60 + g)
        scans = [scan(rng, n) for n in (3000, 28800, 28800)]
        S.compare(f"toggle {on}", S.run(scans, poses_walk(rng, 3, pose), "async"))
    assert S.stable_differs()


def test_unknown_values_are_refused(gpu):
    eng = gpu.Engine(4.0, 4.0, 0.5)
    for bad in (-1, 2):
        with pytest.raises(Exception):
            eng.set_option("voxel_any_order", bad)
