"""fdm_cloud_voxel_grid (CENTROID, NEAREST, ANY, CENTER) and fdm_cloud_grid_max_z through the C ABI against
tests/voxel_restate.py: every output channel and idx BIT for bit, at both orders, with host and with device inputs.

The clouds are chosen for where the kernels can break: point counts around the wavefront, the block and the sort tile;
run lengths across the 256-position block of the run finder and the introsort's 16 / 2048 thresholds; one voxel, one
voxel per point; dropped points; keys at the clamp and beyond the int range; ties whose winner depends on the order.
Where order 1 is checked the clouds stay under 5 000 points (the Python model of std::sort is slow)."""
import ctypes as C

import numpy as np
import pytest

import voxel_restate as V

pytestmark = pytest.mark.gpu
F32 = np.float32
MODES = ("centroid", "nearest", "any", "center", "max_z")
NAMES = ("x", "y", "z", "intensity", "rgb", "nx", "ny", "nz", "cov9")


@pytest.fixture(scope="module")
def fdm():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import fastdem_amd
    fastdem_amd.capi.load()
    return fastdem_amd


# ---- the clouds: dict of channels (absent = None) ----
def with_channels(x, y, z, seed=0, which=("intensity", "rgb", "normals", "cov9")):
    rng = np.random.default_rng(seed + 1000)
    n = x.size
    ch = {k: None for k in NAMES}
    ch["x"], ch["y"], ch["z"] = (np.ascontiguousarray(a, dtype=F32) for a in (x, y, z))
    if "intensity" in which:
        ch["intensity"] = rng.uniform(0, 255, n).astype(F32)
    if "rgb" in which:
        ch["rgb"] = rng.integers(0, 1 << 24, n).astype(np.uint32)
    if "normals" in which:
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        ch["nx"], ch["ny"], ch["nz"] = (np.ascontiguousarray(v[:, k], dtype=F32) for k in range(3))
    if "cov9" in which:
        ch["cov9"] = rng.uniform(-1, 1, (n, 9)).astype(F32)
    return ch


def tied(n, cells, seed, span=2.0):
    """n points in about `cells` voxels of 0.25 m, around the origin (negative coordinates included)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, max(1, cells), n)
    side = max(1, int(round(max(1, cells) ** (1 / 3))))
    x = (c % side) * 0.25 + rng.uniform(0.01, 0.24, n) - span / 2
    y = ((c // side) % side) * 0.25 + rng.uniform(0.01, 0.24, n) - span / 2
    z = (c // (side * side)) * 0.25 + rng.uniform(0.01, 0.24, n) - 0.5
    return x.astype(F32), y.astype(F32), z.astype(F32)


def runs_cloud(lengths, seed, shuffle=True):
    """One voxel of 0.25 m per entry of `lengths`, that many points in it, in shuffled input order."""
    rng = np.random.default_rng(seed)
    v = np.repeat(np.arange(len(lengths)), lengths)
    if shuffle:
        v = rng.permutation(v)
    n = v.size
    x = ((v % 5) * 0.25 + rng.uniform(0.01, 0.24, n) - 0.5).astype(F32)
    y = ((v // 5) * 0.25 + rng.uniform(0.01, 0.24, n) - 0.25).astype(F32)
    z = rng.uniform(0.01, 0.24, n).astype(F32)
    return x, y, z


RUN_LENGTHS = [1, 2, 16, 17, 64, 65, 256, 257, 513, 2049]


def far_cloud(size, seed):
    """Coordinates that are negative, at the +-2^20 clamp of the key, and beyond the int32 range."""
    rng = np.random.default_rng(seed)
    edge = F32(1 << 20) * F32(size)
    vals = np.asarray([0.0, -0.0, 0.3 * size, -0.3 * size, -3.7 * size, 3.7 * size, edge, -edge,
                       np.nextafter(edge, F32(0)), np.nextafter(-edge, F32(0)), edge * F32(2), -edge * F32(2),
                       2.2e9 * size, -2.2e9 * size, 1e30, -1e30, 3.0e38, -3.0e38], dtype=F32)
    pick = lambda: vals[rng.integers(0, vals.size, 900)]  # noqa: E731
    return pick(), pick(), pick()


# ---- through the C ABI ----
def call_abi(fdm, ch, size, mode, order, on_device, device=0, only=None):
    """(rc, n_out, dict of output arrays as numpy) of fdm_cloud_voxel_grid / fdm_cloud_grid_max_z."""
    import torch
    lib = fdm.capi.load()
    n = ch["x"].size
    present = [k for k in NAMES if ch[k] is not None]
    wanted = [k for k in present + ["idx"] if only is None or k in only]
    shape = lambda k: (n, 9) if k == "cov9" else (n,)  # noqa: E731
    dtype = lambda k: np.uint32 if k in ("rgb", "idx") else F32  # noqa: E731
    keep = []
    if on_device:
        def dev(a):
            t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()
            keep.append(t)
            return C.c_void_p(t.data_ptr())
        src = {k: dev(ch[k]) for k in present}
        outs = {k: torch.full(shape(k), -7, dtype=torch.int32 if dtype(k) == np.uint32 else torch.float32, device="cuda")
                for k in wanted}
        torch.cuda.synchronize()
        dst = {k: C.c_void_p(t.data_ptr()) for k, t in outs.items()}
    else:
        src = {k: np.ascontiguousarray(ch[k]) for k in present}
        keep.extend(src.values())
        src = {k: a.ctypes.data_as(C.c_void_p) for k, a in src.items()}
        outs = {k: np.full(shape(k), -7).astype(dtype(k)) for k in wanted}
        dst = {k: a.ctypes.data_as(C.c_void_p) for k, a in outs.items()}
    view = fdm.capi.FdmCloudView(**src)
    out = fdm.capi.FdmCloudOut(**dst)
    n_out = C.c_uint64(12345)
    size = float(size) if isinstance(size, float) and np.isnan(size) else float(F32(size))
    if mode == "max_z":
        rc = lib.fdm_cloud_grid_max_z(n, C.byref(view), int(on_device), size, order, device, C.byref(out), C.byref(n_out))
    else:
        rc = lib.fdm_cloud_voxel_grid(n, C.byref(view), int(on_device), size, V.MODES.index(mode), order, device,
                                      C.byref(out), C.byref(n_out))
    if on_device:
        outs = {k: t.cpu().numpy().view(dtype(k)) for k, t in outs.items()}
    return rc, int(n_out.value), outs


def restate(ch, size, mode, order):
    nrm = None if ch["nx"] is None else (ch["nx"], ch["ny"], ch["nz"])
    kw = dict(intensity=ch["intensity"], rgb=ch["rgb"], normals=nrm, cov=ch["cov9"], order=order)
    if mode == "max_z":
        return V.grid_max_z(ch["x"], ch["y"], ch["z"], size, **kw)
    return V.voxel_grid(ch["x"], ch["y"], ch["z"], size, mode, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(fdm, ch, size, modes=MODES, orders=(0, 1), inputs=(0, 1), expect_n=None):
    """Every mode x order x (host, device) of one cloud against the restatement; returns the restated outputs."""
    wants = {}
    for mode in modes:
        for order in orders:
            want = wants[mode, order] = restate(ch, size, mode, order)
            if expect_n is not None:
                assert want["idx"].size == expect_n
            for on_device in inputs:
                rc, n_out, got = call_abi(fdm, ch, size, mode, order, on_device)
                tag = f"{mode} order {order} {'device' if on_device else 'host'}"
                assert rc == 0, (tag, fdm.capi.load().fdm_last_error())
                assert n_out == want["idx"].size, (tag, n_out, want["idx"].size)
                for k, a in got.items():
                    w = want[k]
                    assert w is not None, (tag, k)
                    bad = np.flatnonzero((bits(a[:n_out]) != bits(w)).reshape(n_out, -1).any(axis=1)) if n_out else []
                    bad = np.asarray(bad, dtype=np.int64)
                    assert bad.size == 0, f"{tag}: {k} differs in {bad.size} of {n_out} outputs, first at {bad[:5]}: " \
                                          f"{a[bad[:3]]} vs {w[bad[:3]]}"
                    assert (bits(a[n_out:]) == bits(np.full(1, -7).astype(a.dtype))[0]).all(), f"{tag}: {k} written past n_out"
    return wants


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1024, 1025])
def test_point_counts(fdm, n):
    x, y, z = tied(n, max(1, n // 4), seed=n)
    check(fdm, with_channels(x, y, z, seed=n), 0.25)


def test_run_lengths_across_the_block_and_the_introsort_thresholds(fdm):
    x, y, z = runs_cloud(RUN_LENGTHS, seed=1)
    wants = check(fdm, with_channels(x, y, z, seed=1), 0.25, expect_n=len(RUN_LENGTHS))
    got = sorted(np.diff(np.append(V.sorted_runs(x, y, z, 0.25)[2], x.size)).tolist())
    assert got == RUN_LENGTHS
    assert not np.array_equal(wants["any", 0]["idx"], wants["any", 1]["idx"])


def test_run_lengths_in_sorted_input_order(fdm):
    """The same runs arriving voxel by voxel: every run but the last starts inside another block than it ends in."""
    x, y, z = runs_cloud(RUN_LENGTHS, seed=2, shuffle=False)
    check(fdm, with_channels(x, y, z, seed=2, which=("intensity",)), 0.25, expect_n=len(RUN_LENGTHS))


def test_run_lengths_around_the_lane_batch_and_the_wavefront_threshold(fdm):
    """Runs are walked four entries at a time by one lane up to 128 entries, by a wavefront, 64 at a time, beyond."""
    lengths = [3, 4, 5, 7, 8, 9, 127, 128, 129, 130, 191, 192, 193]
    x, y, z = runs_cloud(lengths, seed=16)
    check(fdm, with_channels(x, y, z, seed=16), 0.25, expect_n=len(lengths))


def test_all_points_in_one_voxel(fdm):
    rng = np.random.default_rng(3)
    x, y, z = (rng.uniform(0.01, 0.99, 1500).astype(F32) for _ in range(3))
    check(fdm, with_channels(x, y, z, seed=3), 1.0, expect_n=1)


def test_every_point_in_its_own_voxel(fdm):
    rng = np.random.default_rng(4)
    cell = rng.permutation(4000)[:1000]
    x = ((cell % 20) * 0.25 + 0.1).astype(F32) - F32(2.0)
    y = ((cell // 20 % 20) * 0.25 + 0.1).astype(F32) - F32(2.0)
    z = ((cell // 400) * 0.25 + 0.1).astype(F32)
    check(fdm, with_channels(x, y, z, seed=4), 0.25, modes=("centroid", "nearest", "any", "center"), expect_n=1000)
    wants = check(fdm, with_channels(x, y, z, seed=4), 0.25, modes=("max_z",))
    assert 300 < wants["max_z", 0]["idx"].size <= 400                 # (one (x, y) cell per column of voxels)


def test_non_finite_points_are_dropped(fdm):
    x, y, z = tied(2000, 150, seed=5)
    rng = np.random.default_rng(5)
    x[rng.random(2000) < 0.05] = np.nan
    y[rng.random(2000) < 0.05] = np.inf
    z[rng.random(2000) < 0.05] = -np.inf
    z[rng.random(2000) < 0.03] = np.nan
    x[0] = np.nan
    z[-1] = np.inf
    ch = with_channels(x, y, z, seed=5)
    wants = check(fdm, ch, 0.25)
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    assert 0 < ok.sum() < 2000 and ok[wants["nearest", 0]["idx"]].all()


def test_a_cloud_without_a_finite_point_gives_nothing(fdm):
    x, y, z = tied(300, 20, seed=6)
    x[0::3] = np.nan
    y[1::3] = np.inf
    z[2::3] = -np.inf
    check(fdm, with_channels(x, y, z, seed=6), 0.25, expect_n=0)


@pytest.mark.parametrize("size", [0.001, 0.05, 100.0])
def test_negative_clamped_and_beyond_int_coordinates(fdm, size):
    x, y, z = far_cloud(size, seed=7)
    wants = check(fdm, with_channels(x, y, z, seed=7, which=("intensity", "rgb")), size)
    ix = V.unpack(V.keys_of(x, y, z, size)[1])[0]
    assert (ix == -(1 << 20)).any() and (ix == (1 << 20) - 1).any() and ((ix < 0) & (ix > -100)).any()
    assert 1 < wants["center", 0]["idx"].size < x.size


def test_size_limits(fdm):
    x, y, z = tied(100, 10, seed=8)
    ch = with_channels(x, y, z, seed=8, which=())
    for size in (0.001, 100.0):
        check(fdm, ch, size, orders=(0,))
    lib = fdm.capi.load()
    for size in (0.0009, 100.5, float("nan")):
        for mode in MODES:
            for on_device in (0, 1):
                rc, n_out, got = call_abi(fdm, ch, size, mode, 0, on_device)
                assert rc == fdm.capi.FDM_ERR_INVALID and n_out == 0
                text = "grid_size" if mode == "max_z" else "voxel_size"
                assert lib.fdm_last_error().decode() == f"{text} must be in [0.001, 100]"
                assert (got["x"] == -7).all()


def test_refused_arguments_and_the_empty_cloud(fdm):
    lib = fdm.capi.load()
    x, y, z = tied(50, 5, seed=9)
    ch = with_channels(x, y, z, seed=9, which=("normals",))
    for bad in (dict(mode=4), dict(mode=-1), dict(order=2), dict(order=-1)):
        view = fdm.capi.FdmCloudView(**{k: ch[k].ctypes.data_as(C.c_void_p) for k in ("x", "y", "z")})
        n_out = C.c_uint64(5)
        rc = lib.fdm_cloud_voxel_grid(50, C.byref(view), 0, 0.25, bad.get("mode", 0), bad.get("order", 0), 0, None,
                                      C.byref(n_out))
        assert rc == fdm.capi.FDM_ERR_INVALID and n_out.value == 0, bad
    n_out = C.c_uint64(5)
    assert lib.fdm_cloud_grid_max_z(50, C.byref(view), 0, 0.25, 3, 0, None, C.byref(n_out)) == fdm.capi.FDM_ERR_INVALID
    for n in ((1 << 32) - 4096, (1 << 32) - 2, 1 << 40):
        assert lib.fdm_cloud_voxel_grid(n, C.byref(view), 0, 0.25, 0, 0, 0, None, C.byref(n_out)) == fdm.capi.FDM_ERR_INVALID
    partial = dict(ch, ny=None)
    rc, n_out, _ = call_abi(fdm, partial, 0.25, "centroid", 0, 0)
    assert rc == fdm.capi.FDM_ERR_INVALID and n_out == 0 and b"normals" in lib.fdm_last_error()
    n_out = C.c_uint64(5)
    assert lib.fdm_cloud_voxel_grid(0, None, 0, 0.25, 0, 0, 0, None, C.byref(n_out)) == 0 and n_out.value == 0
    n_out = C.c_uint64(5)
    assert lib.fdm_cloud_grid_max_z(0, None, 1, 0.25, 1, 0, None, C.byref(n_out)) == 0 and n_out.value == 0
    # outputs are optional one by one: idx alone, and none at all (a count)
    for mode in MODES:
        want = restate(ch, 0.25, mode, 0)
        rc, n, got = call_abi(fdm, ch, 0.25, mode, 0, 1, only=("idx",))
        assert rc == 0 and sorted(got) == ["idx"] and np.array_equal(got["idx"][:n], want["idx"])
        rc, n, got = call_abi(fdm, ch, 0.25, mode, 0, 0, only=())
        assert rc == 0 and n == want["idx"].size and not got
        # ... and so is each of the three normal arrays: one alone, host and device
        for one in ("nx", "ny", "nz"):
            for on_device in (0, 1):
                rc, n, got = call_abi(fdm, ch, 0.25, mode, 0, on_device, only=(one,))
                assert rc == 0 and n == want["idx"].size and sorted(got) == [one]
                assert np.array_equal(bits(got[one][:n]), bits(want[one])), (mode, one, on_device)
                assert (got[one][n:] == -7).all()


def test_ties_inside_long_runs_follow_the_order(fdm):
    """Runs of 17 and more equal keys whose points are all EQUALLY near the centre and equally high: NEAREST and gridMaxZ
    keep the first of the run, which std::sort's order and the stable order disagree on."""
    lengths = [17, 40, 90, 300, 20, 33]
    rng = np.random.default_rng(10)
    v = rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    x = (v * 0.25 + 0.05).astype(F32)
    y = np.full(v.size, 0.2, dtype=F32)
    z = np.full(v.size, 0.1, dtype=F32)
    ch = with_channels(x, y, z, seed=10, which=("intensity",))
    ch["intensity"] = np.arange(v.size, dtype=F32)
    wants = check(fdm, ch, 0.25, expect_n=len(lengths))
    for mode in ("nearest", "max_z"):
        assert not np.array_equal(wants[mode, 0]["idx"], wants[mode, 1]["idx"]), mode
        assert not np.array_equal(wants[mode, 0]["intensity"], wants[mode, 1]["intensity"]), mode
    first = np.asarray([np.flatnonzero(v == k)[0] for k in range(len(lengths))])
    assert np.array_equal(wants["nearest", 0]["idx"], first) and np.array_equal(wants["max_z", 0]["idx"], first)
    # ... and ties only among SOME of a run: a strictly better point later in the run still wins in both orders
    z2 = z.copy()
    best = np.asarray([np.flatnonzero(v == k)[-1] for k in range(len(lengths))])
    z2[best] = 0.125                                                  # the voxel's centre height, and its highest point
    wants = check(fdm, dict(ch, z=z2), 0.25, modes=("nearest", "max_z"))
    for key in wants:
        assert np.array_equal(wants[key]["idx"], best), key


def test_a_colour_mean_truncates(fdm):
    x, y, z = (np.full(3, 0.1, dtype=F32) for _ in range(3))
    ch = with_channels(x, y, z, which=())
    ch["rgb"] = np.asarray([0x0A00FF, 0x0B01FF, 0x0B01FE], dtype=np.uint32)       # means 10.67, 0.67, 254.67
    wants = check(fdm, ch, 1.0, modes=("centroid", "center"))
    assert wants["centroid", 0]["rgb"].tolist() == [0x0A00FE]


def test_opposite_normals_give_unit_z(fdm):
    x = np.asarray([0.1, 0.2, 0.6, 0.7], dtype=F32)
    y, z = np.full(4, 0.1, dtype=F32), np.full(4, 0.1, dtype=F32)
    ch = with_channels(x, y, z, which=())
    ch["nx"] = np.asarray([1, -1, 0.6, 0.6], dtype=F32)
    ch["ny"] = np.asarray([0, 0, 0.8, 0.8], dtype=F32)
    ch["nz"] = np.asarray([0, 0, 0, 0], dtype=F32)
    wants = check(fdm, ch, 0.5, modes=("centroid", "center"))
    w = wants["centroid", 0]
    assert (w["nx"][0], w["ny"][0], w["nz"][0]) == (0.0, 0.0, 1.0)
    assert abs(float(w["nx"][1]) - 0.6) < 1e-6 and abs(float(w["ny"][1]) - 0.8) < 1e-6 and w["nz"][1] == 0.0


@pytest.mark.parametrize("which", [(), ("intensity",), ("rgb",), ("normals",), ("cov9",),
                                   ("intensity", "rgb", "normals", "cov9")],
                         ids=["none", "intensity", "rgb", "normals", "cov9", "all"])
def test_channel_subsets(fdm, which):
    x, y, z = tied(700, 60, seed=12)
    check(fdm, with_channels(x, y, z, seed=12, which=which), 0.25)


def test_any_is_what_fdm_engine_voxel_any_returns(fdm):
    x, y, z = tied(3000, 300, seed=13)
    ch = with_channels(x, y, z, which=())
    eng = fdm.Engine(4.0, 4.0, 0.5)
    for order in (0, 1):
        eng.set_option("voxel_any_order", order)
        rc, n, got = call_abi(fdm, ch, 0.25, "any", order, 0)
        assert rc == 0 and np.array_equal(got["idx"][:n], eng.voxel_any(x, y, z, 0.25))
    eng.close()


def test_600001_points_cross_the_4096_pair_sort_tile(fdm):
    """Order 0 only.  Voxels of about eight points; every mode, CENTROID and NEAREST with host and with device input."""
    n = 600001
    x, y, z = tied(n, n // 8, seed=14, span=10.0)
    x[::1000] = np.nan
    ch = with_channels(x, y, z, seed=14, which=("intensity", "rgb", "normals"))
    check(fdm, ch, 0.25, modes=("centroid", "nearest"), orders=(0,))
    check(fdm, ch, 0.25, modes=("center",), orders=(0,), inputs=(0,))
    check(fdm, ch, 0.25, modes=("any", "max_z"), orders=(0,), inputs=(1,))


# ---- the Python surface ----
def test_python_torch_tensors_equal_the_numpy_path(fdm):
    import torch
    x, y, z = tied(3000, 250, seed=15)
    ch = with_channels(x, y, z, seed=15)
    nrm = (ch["nx"], ch["ny"], ch["nz"])
    t = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in ch.items()}
    for mode in MODES:
        for order in (0, 1):
            if mode == "max_z":
                a = fdm.grid_max_z(x, y, z, 0.25, intensity=ch["intensity"], rgb=ch["rgb"], normals=nrm, cov=ch["cov9"],
                                   order=order, return_index=True)
                b = fdm.grid_max_z(t["x"], t["y"], t["z"], 0.25, intensity=t["intensity"], rgb=t["rgb"],
                                   normals=(t["nx"], t["ny"], t["nz"]), cov=t["cov9"], order=order, return_index=True)
            else:
                a = fdm.voxel_grid(x, y, z, 0.25, mode, intensity=ch["intensity"], rgb=ch["rgb"], normals=nrm,
                                   cov=ch["cov9"], order=order, return_index=True)
                b = fdm.voxel_grid(t["x"], t["y"], t["z"], 0.25, mode, intensity=t["intensity"], rgb=t["rgb"],
                                   normals=(t["nx"], t["ny"], t["nz"]), cov=t["cov9"], order=order, return_index=True)
            want = restate(ch, 0.25, mode, order)
            assert sorted(a) == sorted(b) == ["cov", "idx", "intensity", "normals", "rgb", "x", "y", "z"]
            assert a["x"].size == want["idx"].size and b["x"].is_cuda
            for k in ("x", "y", "z", "intensity", "rgb", "cov", "idx"):
                got_t = b[k].cpu().numpy()
                assert np.array_equal(bits(a[k]) if k != "idx" else a[k], bits(got_t) if k != "idx" else got_t), (mode, k)
                assert np.array_equal(bits(a[k]), bits(want["cov9" if k == "cov" else k])), (mode, k)
            for q, k in enumerate(("nx", "ny", "nz")):
                assert np.array_equal(bits(a["normals"][q]), bits(b["normals"][q].cpu().numpy()))
                assert np.array_equal(bits(a["normals"][q]), bits(want[k]))
    # the result feeds the rasterizer without leaving the device
    b = fdm.voxel_grid(t["x"], t["y"], t["z"], 0.25, "centroid", intensity=t["intensity"])
    eng = fdm.from_point_cloud(b["x"], b["y"], b["z"], 0.25, intensity=b["intensity"])
    assert eng is not None
    eng.close()
