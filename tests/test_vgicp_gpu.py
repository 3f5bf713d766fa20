"""Voxelized GICP on the device (fastdem_amd/csrc/fdm_vgicp.hpp; fdm_voxel_map_create, fdm_cloud_register_vgicp and
fdm_cloud_register_vgicp_linearize) against the NumPy restatement of nanoPCL's VoxelDistributionMap and alignVGICP
(tests/vgicp_restate.py).

The map's keys, counts, means and covariances are held BIT FOR BIT: the sums are sequential in input order on both sides.
C_reg is held within 1e-12 absolute: two double eigen-solvers differ by about 10 eps |C| / gap in v0, which with the
relative gap >= 0.25 every such test first asserts on the restatement alone is under 1e-14 in v0 v0T — a hundredfold
margin.  A linearization is held to the same inliers, the same correspondences and every one of the 28 sums within 1e-9
sum|term|, the bound tests/test_register_gpu.py uses for GICP for the same reason.  align is held on the cases
tests/test_vgicp_restate.py admits: the same iterations, converged and fitness, the transform and rmse within 64 x the
case's recorded spread between summation orders (floor 1e-13).

Run on the GPU box:  python -m pytest tests -m gpu
"""
import ctypes as C
import math

import numpy as np
import pytest

import reg_cases as RC
import reg_restate as RR
import vgicp_cases as VC
import vgicp_restate as VG

pytestmark = pytest.mark.gpu
F32 = np.float32
KERNEL_NAMES = {RR.NONE: "none", RR.HUBER: "huber", RR.TUKEY: "tukey", RR.CAUCHY: "cauchy"}
CREG_TOL = 1e-12


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check_map(gpu, cloud, resolution, label, eps=1e-3, tight=True, on_device=False):
    """Build on the device, compare with the restatement; returns (restated map, info)."""
    want = VG.Map(*cloud, resolution, eps)
    if tight:
        VC.assert_gaps(want)
    src = cloud
    if on_device:
        import torch
        src = [torch.from_numpy(np.array(v, dtype=F32)).cuda() for v in cloud]
    with gpu.VoxelMap(*src, resolution=resolution, covariance_epsilon=eps) as vm:
        info, rec = vm.info(), vm.records()
    assert info["n_points"] == want.n_points and info["n_skipped"] == want.n_skipped, (label, info)
    assert info["num_voxels"] == want.num_voxels == len(rec["key"]), (label, info)
    assert np.array_equal(rec["key"], want.key), label
    assert np.array_equal(rec["count"], want.count), label
    assert np.array_equal(bits(rec["mean"]), bits(want.mean)), (label, np.flatnonzero((bits(rec["mean"]) != bits(want.mean)).any(axis=1)))
    assert np.array_equal(bits(rec["cov"]), bits(want.cov)), (label, np.flatnonzero((bits(rec["cov"]) != bits(want.cov)).any(axis=(1, 2))))
    assert info["n_sparse"] == int((want.count < 3).sum()), (label, info)
    assert info["max_count"] == (int(want.count.max()) if want.num_voxels else 0), (label, info)
    sparse = want.count < 3
    assert np.array_equal(rec["creg"][sparse], np.tile(np.eye(3), (int(sparse.sum()), 1, 1))), label   # exactly I
    worst = float(np.abs(rec["creg"] - want.creg).max()) if want.num_voxels else 0.0
    print(f"{label}: {want.n_points} points, {want.num_voxels} voxels ({int(want.full.sum())} full, fullest "
          f"{info['max_count']}), skipped {want.n_skipped}, smallest gap {want.min_gap():.3g}, C_reg off by {worst:.3g}; "
          f"table {info['table_slots']} slots, longest probe {info['max_probe']}")
    if tight:
        assert worst <= CREG_TOL, label
    if want.num_voxels:
        assert info["table_slots"] >= 2 * want.num_voxels and info["table_slots"] & (info["table_slots"] - 1) == 0
        assert 1 <= info["max_probe"] <= want.num_voxels
    else:
        assert info["table_slots"] == 0 and info["max_probe"] == 0
    assert info["ms"] == (0.0, 0.0, 0.0)                             # no events unless fdm_cloud_debug_profile is on
    return want, rec


def cloud_of(points):
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    return tuple(np.ascontiguousarray(p[:, a]) for a in range(3))


def discs(n_voxels, m, seed, extra=0):
    """n_voxels voxels of m points each (a disc for m >= 3), and `extra` further points of their own elsewhere."""
    c = VC.designed(n_voxels, (m,), seed)
    if not extra:
        return c
    g = np.random.default_rng(seed + 1)
    far = (g.choice(40 ** 3, size=extra, replace=False)[:, None] // np.array([1, 40, 1600]) % 40 + 20.25) * VC.EDGE
    return tuple(np.concatenate([a, far[:, k].astype(F32)]) for k, a in enumerate(c))


# ---- 1. the map's records ----
def test_map_of_the_designed_cloud(gpu):
    want, _ = check_map(gpu, VC.designed(500), VC.EDGE, "designed 500")
    assert want.count.max() > 128 and (want.count < 3).any() and (want.key < (1 << 20 << 42)).any()   # long runs, sparse, z < 0


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_map_of_single_point_voxels(gpu, n):
    """Every point its own voxel: the run heads at a block's edge."""
    check_map(gpu, discs(n, 1, 3), VC.EDGE, f"{n} voxels of 1")


@pytest.mark.parametrize("n", [255, 256, 257])
def test_map_of_three_point_voxels(gpu, n):
    want, _ = check_map(gpu, discs(n, 3, 4), VC.EDGE, f"{n} voxels of 3")
    assert want.full.all()


@pytest.mark.parametrize("m", [128, 129, 300])
def test_map_with_one_long_voxel(gpu, m):
    """Either side of the run length that goes to a wavefront, with 4 000 further points elsewhere."""
    want, _ = check_map(gpu, discs(1, m, 5, extra=4000), VC.EDGE, f"one voxel of {m}")
    assert want.count.max() == m and want.num_voxels == 4001


def test_map_of_a_cloud_in_one_voxel(gpu):
    want, _ = check_map(gpu, discs(1, 2000, 6), VC.EDGE, "2000 in one voxel")
    assert want.num_voxels == 1


def test_map_skips_points_that_are_not_finite(gpu):
    c = np.stack(VC.designed(300, (1, 2, 3, 4, 5, 8)), axis=1)
    bad = c[:90].copy()                                              # 90 further points, one coordinate of each not finite
    bad[np.arange(90), np.arange(90) % 3] = np.array([np.nan, np.inf, -np.inf], dtype=F32)[np.arange(90) // 3 % 3]
    at = np.sort(np.random.default_rng(9).integers(0, c.shape[0] + 1, size=90))
    mixed = np.insert(c, at, bad, axis=0)                            # interleaved: the voxels' own points stay in order
    want, _ = check_map(gpu, cloud_of(mixed), VC.EDGE, "with NaN and Inf")
    assert want.n_skipped == 90 and want.num_voxels == 300
    bad = tuple(np.full(40, v, dtype=F32) for v in (np.nan, 1.0, np.inf))
    empty, _ = check_map(gpu, bad, VC.EDGE, "nothing finite")
    assert empty.num_voxels == 0 and empty.n_skipped == 40
    none, _ = check_map(gpu, tuple(np.zeros(0, dtype=F32) for _ in range(3)), VC.EDGE, "n = 0")
    assert none.num_voxels == 0


def test_map_of_negative_coordinates_multiples_of_the_edge_and_minus_zero(gpu):
    g = np.random.default_rng(8)
    k = np.arange(-6, 7, dtype=np.float64)
    on = np.stack(np.meshgrid(k, k[:3], k[:2], indexing="ij"), axis=-1).reshape(-1, 3) * 0.5     # exactly on voxel faces
    near = -np.abs(g.uniform(0.0, 3.0, size=(200, 3)))
    want, rec = check_map(gpu, cloud_of(np.concatenate([on, near])), 0.5, "faces and negatives", tight=False)
    # a voxel whose points all have x = -0.0f keeps a -0.0 sum (the first point is assigned, not added to zero)
    p = np.array([[-0.0, 0.1, 0.1], [-0.0, 0.2, 0.3], [-0.0, 0.4, 0.2], [-0.0, 0.3, 0.45]], dtype=F32)
    for n in (1, 2, 3, 4):
        want, rec = check_map(gpu, cloud_of(p[:n]), 0.5, f"minus zero x {n}", tight=False)
        assert want.num_voxels == 1 and np.signbit(want.mean[0, 0]) and np.signbit(rec["mean"][0, 0])


def test_map_clamps_keys(gpu):
    """resolution 0.001 and |x| = 2 000: the index is clamped to +-2^20."""
    pts = [[2000.0, 0.0, 0.0], [2000.5, 0.0004, 0.0], [1999.0, 0.0002, 0.0002], [-2000.0, 0.0, 0.0], [-3000.0, 0.0, 0.0],
           [0.0, 2000.0, -2000.0], [0.0001, 0.0001, 0.0001], [1e30, -1e30, 1e30]]
    want, _ = check_map(gpu, cloud_of(pts), 0.001, "clamped", tight=False)
    assert want.num_voxels == 5 and want.count.max() == 3


def test_host_and_device_inputs_give_the_same_bytes(gpu):
    c = VC.designed(300, (1, 2, 3, 4, 5, 8))
    _, a = check_map(gpu, c, VC.EDGE, "host")
    _, b = check_map(gpu, c, VC.EDGE, "device", on_device=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_map_refusals(gpu):
    c = VC.designed(300, (1, 2, 3, 4, 5, 8))
    for res in (0.0, -1.0, math.nan, math.inf, 1e-39):                 # 1.0f / 1e-39f is not finite
        with pytest.raises(gpu.EngineError):
            gpu.VoxelMap(*c, resolution=res)
    for eps in (-1e-3, math.nan):
        with pytest.raises(gpu.EngineError):
            gpu.VoxelMap(*c, covariance_epsilon=eps)


# ---- 2. the hash ----
def check_lookup(gpu, target, queries, label):
    want_map = VG.Map(*target, VC.EDGE)
    want = want_map.rank_of(np.stack(queries, axis=1))
    cov = np.tile(np.eye(3, dtype=F32), (queries[0].size, 1, 1))
    with gpu.VoxelMap(*target, resolution=VC.EDGE) as vm:
        info = vm.info()
        got = gpu.linearize_vgicp(*queries, cov, voxel_map=vm, return_correspondences=True)
        st = gpu.register_last_stats()
    print(f"{label}: {info['num_voxels']} voxels, table {info['table_slots']} slots, longest probe {info['max_probe']}")
    assert info["max_probe"] <= info["num_voxels"]
    assert np.array_equal(got["corr"].astype(np.int64), want), label
    assert got["num_inliers"] == int((want >= 0).sum())
    assert (st["n_source"], st["n_target"], st["grid_x"], st["grid_y"], st["ring_limit"], st["linearizations"]) == \
        (queries[0].size, info["num_voxels"], 0, 0, 0, 1), st
    assert st["voxel"] == F32(VC.EDGE) and st["ms"] == (0.0, 0.0, 0.0)
    return want


def line_of_voxels(n, axis, start=-150):
    """n voxels in a row along `axis`, three points each, shuffled."""
    g = np.random.default_rng(20 + axis)
    idx = np.zeros((n, 3))
    idx[:, axis] = np.arange(start, start + n)
    idx[:, (axis + 1) % 3], idx[:, (axis + 2) % 3] = 3, -2
    p = ((idx[:, None, :] + g.uniform(0.1, 0.9, size=(n, 3, 3))) * VC.EDGE).reshape(-1, 3)
    return cloud_of(p[g.permutation(p.shape[0])])


@pytest.mark.parametrize("axis,name", [(2, "a vertical column"), (0, "a row along x")])
def test_lookup_in_a_line_of_voxels(gpu, axis, name):
    """300 voxels with the same (x, y), keys that differ only in z — what `key & mask` would put into one slot — and 300
    along x; the target itself as source, shuffled."""
    t = line_of_voxels(300, axis)
    want = check_lookup(gpu, t, t, name)
    assert (want >= 0).all() and np.unique(want).size == 300


def test_lookup_of_keys_that_differ_only_above_bit_32(gpu):
    """y's upper bits and z: x and the low 11 bits of y are the same in all 300 keys."""
    g = np.random.default_rng(23)
    idx = np.zeros((300, 3))
    idx[:, 1] = (np.arange(300) % 20 - 10) * 2048 + 5
    idx[:, 2] = np.arange(300) // 20 - 7
    p = ((idx[:, None, :] + g.uniform(0.25, 0.75, size=(300, 3, 3))) * VC.EDGE).reshape(-1, 3)
    t = cloud_of(p[g.permutation(p.shape[0])])
    want_map = VG.Map(*t, VC.EDGE)
    assert want_map.num_voxels == 300 and np.unique(want_map.key & np.uint64(0xFFFFFFFF)).size == 1
    want = check_lookup(gpu, t, t, "keys equal below bit 32")
    assert (want >= 0).all()


def test_lookup_misses_next_to_occupied_voxels_and_finds_sparse_ones(gpu):
    t = VC.designed(300, (1, 2, 3, 4, 5, 8))
    m = VG.Map(*t, VC.EDGE)
    ix, iy, iz = VG.VR.unpack(m.key)
    centres = (np.stack([ix, iy, iz], axis=1) + 0.5) * VC.EDGE
    q = np.concatenate([centres + np.array(d) * VC.EDGE for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1))] + [centres])
    want = check_lookup(gpu, t, cloud_of(q), "neighbours and centres")
    assert (want < 0).sum() > 600 and (want[-300:] == np.arange(300)).all()
    assert (m.count[want[-300:]] < 3).any()                          # sparse voxels are found


# ---- 3. linearize against the restatement ----
def check_linearize(gpu, vm, problem, T, label):
    want = problem.linearize(T)
    got = gpu.linearize_vgicp(*problem.s, problem.source_cov, voxel_map=vm, transform=T, return_correspondences=True,
                              **problem.set)
    assert got["num_inliers"] == want["num_inliers"], label
    assert np.array_equal(got["corr"].astype(np.int64), want["corr"]), label
    sums = np.concatenate([got["H_upper"], got["b"], [got["error"]]])
    diff = np.abs(sums - want["sums"])
    limit = 1e-9 * want["abs_sums"]
    worst = float(np.max(np.where(limit > 0, diff / np.where(limit > 0, limit, 1.0), np.where(diff > 0, np.inf, 0.0))))
    print(f"{label}: {want['num_inliers']}/{problem.n} inliers, worst sum at {worst:.3g} of its bound")
    assert (diff <= limit).all(), (label, np.flatnonzero(diff > limit), diff, limit)
    return want, got


@pytest.mark.parametrize("kernel", [RR.NONE, RR.HUBER, RR.TUKEY, RR.CAUCHY], ids=lambda k: KERNEL_NAMES[k])
def test_linearize_against_the_restatement(gpu, kernel):
    t, want_map, _ = VC.lin_base()
    VC.assert_gaps(want_map)
    assert want_map.num_voxels == 300
    proper = crossed = 0
    with gpu.VoxelMap(*t, resolution=VC.EDGE) as vm:
        for ns in VC.LIN_SOURCE_SIZES:
            problem = VC.lin_problem(kernel, ns)
            home = want_map.rank_of(np.stack(problem.s, axis=1))
            for ti, T in enumerate(VC.lin_transforms()):
                want, _ = check_linearize(gpu, vm, problem, T, f"{KERNEL_NAMES[kernel]} {ns} T{ti}")
                proper += 0 < want["num_inliers"] < ns
                crossed += int(((want["corr"] >= 0) & (want["corr"] != home)).sum())
    assert proper >= 10 and crossed >= 50                            # points left their voxels: for none, and for another


def test_the_robust_kernels_change_the_sums(gpu):
    t, _, _ = VC.lin_base()
    T = VC.lin_transforms()[0]
    with gpu.VoxelMap(*t, resolution=VC.EDGE) as vm:
        errors = [check_linearize(gpu, vm, VC.lin_problem(k, 1000), T, f"kernel {k}")[1]["error"] for k in range(4)]
    assert len(set(errors)) == 4, errors


def test_device_source_and_two_calls_give_the_same_bits(gpu):
    import torch
    t, _, _ = VC.lin_base()
    problem = VC.lin_problem(RR.HUBER, 1000)
    T = VC.lin_transforms()[1]
    dev = [torch.from_numpy(np.array(v, dtype=F32)).cuda() for v in problem.s]
    dcov = torch.from_numpy(np.array(problem.source_cov, dtype=F32)).cuda()
    with gpu.VoxelMap(*t, resolution=VC.EDGE) as vm:
        a = gpu.linearize_vgicp(*problem.s, problem.source_cov, voxel_map=vm, transform=T, return_correspondences=True, **problem.set)
        b = gpu.linearize_vgicp(*dev, dcov, voxel_map=vm, transform=T, return_correspondences=True, **problem.set)
        c = gpu.linearize_vgicp(*problem.s, problem.source_cov, target=t, voxel_resolution=VC.EDGE, transform=T, **problem.set)
    for k in ("H_upper", "b"):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes()
    assert a["error"] == b["error"] == c["error"] and np.array_equal(a["corr"], b["corr"].cpu().numpy())


# ---- 4. align ----
def check_align(gpu, case, got):
    want = case.restated("forward")
    tol = max(64.0 * case.spread, 1e-13)
    dT = float(np.linalg.norm(got.transform - want.transform))
    print(f"{case.name}: iterations {got.iterations}, fitness {got.fitness:.4f}, rmse {got.rmse:.3e}, transform off by "
          f"{dT:.3e} (bound {tol:.1e})")
    assert (got.iterations, got.converged) == (want.iterations, want.converged)
    assert got.fitness == want.fitness
    assert dT <= tol and abs(got.rmse - want.rmse) <= tol * max(1.0, want.rmse)
    assert (got.covariance is None) == (want.covariance is None)


@pytest.mark.parametrize("name", VC.ALIGN_CASES)
def test_align_against_the_restatement(gpu, name):
    case = VC.align_case(name)
    with gpu.VoxelMap(*case.target, resolution=case.resolution) as vm:
        got = gpu.align_vgicp(*case.source, case.source_cov, voxel_map=vm, **case.settings)
        st = gpu.register_last_stats()
        again = gpu.align_vgicp(*case.source, case.source_cov, voxel_map=vm, **case.settings)   # the map is reusable
    check_align(gpu, case, got)
    assert st["linearizations"] == got.iterations and st["n_target"] == case.map.num_voxels
    assert again.transform.tobytes() == got.transform.tobytes()
    if name == "designed_small":                                      # the convenience form builds and closes a map
        conv = gpu.align_vgicp(*case.source, case.source_cov, target=case.target, voxel_resolution=case.resolution,
                               **case.settings)
        assert conv.transform.tobytes() == got.transform.tobytes()


def test_early_returns_and_refusals(gpu):
    c = VC.designed(300, (1, 2, 3, 4, 5, 8))
    cov = np.tile(np.eye(3, dtype=F32), (c[0].size, 1, 1))
    e = tuple(np.zeros(0, dtype=F32) for _ in range(3))
    guess = RC.translation(1.0, 2.0, 3.0)
    with gpu.VoxelMap(*c, resolution=VC.EDGE) as vm, gpu.VoxelMap(*e, resolution=VC.EDGE) as empty:
        for r in (gpu.align_vgicp(*e, None, voxel_map=vm, initial_guess=guess),          # before the covariances are asked for
                  gpu.align_vgicp(*c, None, voxel_map=empty, initial_guess=guess)):
            assert not r.converged and r.iterations == 0 and r.fitness == 0.0 and math.isinf(r.rmse)
            assert r.covariance is None and np.array_equal(r.transform, guess)
        out = gpu.linearize_vgicp(*c, cov, voxel_map=empty, return_correspondences=True)
        assert out["num_inliers"] == 0 and (out["corr"] == -1).all() and not out["H"].any()
        with pytest.raises(gpu.EngineError, match="source must have covariances"):
            gpu.align_vgicp(*c, None, voxel_map=vm)
        bad = c[0].copy()
        bad[17] = np.nan
        with pytest.raises(gpu.EngineError, match="not finite"):
            gpu.align_vgicp(bad, c[1], c[2], cov, voxel_map=vm)
        with pytest.raises(TypeError):
            gpu.align_vgicp(*c, cov)
        with pytest.raises(TypeError):
            gpu.align_vgicp(*c, cov, voxel_map=vm, target=c)
        far = gpu.align_vgicp(*c, cov, voxel_map=vm, initial_guess=RC.translation(500.0, 0.0, 0.0))   # nobody corresponds
        assert not far.converged and far.iterations == 0 and far.fitness == 0.0
    with pytest.raises(gpu.EngineError, match="closed"):
        vm.info()
    vm.close()                                                        # twice is fine


# ---- 5. the C entries' refusals ----
MSG = {                                                              # the literals of fastdem_amd/csrc, as fdm_last_error() gives them
    "null": "null argument",
    "kernel": "robust_kernel must be 0 (NONE), 1 (HUBER), 2 (TUKEY) or 3 (CAUCHY)",
    "transform": "the transform has an entry that is not finite",
    "count": "point count exceeds 2^31-1",
    "array": "null coordinate array",
    "source_cov": "alignVGICP: source must have covariances",
    "source_finite": "the source cloud has a coordinate that is not finite",
    "device": "the voxel map was built on another device than the source lives on",
}


def test_refusals_say_why_by_both_entries_and_restore_the_device(gpu):
    """Every refusal of fdm_cloud_register_vgicp and fdm_cloud_register_vgicp_linearize: the same code and the same
    fdm_last_error() from both, the earlier fault winning in the order null map, robust_kernel, transform, source cloud,
    (the empty return), source covariances; a null output before all of them; max_correspondence_dist not looked at.  The
    device: where a second one exists the thread is put on it and the map lives on device 0, so a call that did not put
    the thread's device back would leave it on 0; on a machine with one device the assertion cannot fail and proves
    nothing."""
    import torch
    other = torch.cuda.device_count() - 1                            # 0 where there is one device
    torch.cuda.set_device(other)
    lib, INVALID = gpu.capi.load(), gpu.capi.FDM_ERR_INVALID
    c = VC.designed(300, (1, 2, 3, 4, 5, 8))
    n = c[0].size
    keep = [np.ascontiguousarray(v) for v in c] + [np.tile(np.eye(3, dtype=F32), (n, 1, 1))]
    dirty = keep[0].copy()
    dirty[17] = np.nan
    P = [v.ctypes.data_as(C.c_void_p) for v in keep + [dirty]]
    bad_T = np.eye(4).reshape(16).copy()
    bad_T[13] = np.nan
    e = tuple(np.zeros(0, dtype=F32) for _ in range(3))

    def call(vm, ns=n, sx=P[0], cov=P[3], on_device=0, guess=None, null_output=None, **settings):
        st = gpu.align_settings(**settings)
        g = None if guess is None else (C.c_double * 16)(*guess)
        out = [C.byref(gpu.capi.FdmRegistrationResult())]
        lin = [(C.c_double * 21)(), (C.c_double * 6)(), C.byref(C.c_double()), C.byref(C.c_uint64())]
        if null_output is not None:                                  # the align entry's `out`; H, b, error or count
            out[0] = None
            lin[null_output] = None
        h = None if vm is None else vm._handle()
        before = torch.cuda.current_device()
        rc = lib.fdm_cloud_register_vgicp(h, ns, sx, P[1], P[2], cov, on_device, g, C.byref(st), *out)
        said = lib.fdm_last_error().decode()
        rc2 = lib.fdm_cloud_register_vgicp_linearize(h, ns, sx, P[1], P[2], cov, on_device, g, C.byref(st), *lin, None)
        assert (rc2, lib.fdm_last_error().decode()) == (rc, said)
        assert torch.cuda.current_device() == before == other
        return rc, said

    with gpu.VoxelMap(*c, resolution=VC.EDGE, device=0) as vm, gpu.VoxelMap(*e, resolution=VC.EDGE, device=0) as empty:
        refused = lambda key, m=vm, **kw: call(m, **kw) == (INVALID, MSG[key])   # noqa: E731
        assert call(vm)[0] == 0
        assert call(vm, max_correspondence_dist=-1.0)[0] == 0 and call(vm, max_correspondence_dist=math.nan)[0] == 0
        assert refused("null", m=None)
        assert refused("kernel", robust_kernel=4) and refused("kernel", robust_kernel=-1)
        assert refused("transform", guess=bad_T)
        assert refused("count", ns=1 << 31) and refused("array", sx=None)
        assert refused("source_cov", cov=None)
        assert refused("source_finite", sx=P[4])
        # two faults at once
        assert refused("null", m=None, robust_kernel=4, guess=bad_T, sx=None, cov=None)
        assert refused("kernel", robust_kernel=4, guess=bad_T)
        assert refused("transform", guess=bad_T, sx=None)
        assert refused("array", sx=None, cov=None)
        assert refused("source_cov", sx=P[4], cov=None)
        for k in range(4):
            assert refused("null", null_output=k) and refused("null", null_output=k, robust_kernel=4, guess=bad_T)
            assert refused("null", m=None, null_output=k)
        # an empty source or map returns before the covariances are asked for
        assert call(empty, cov=None)[0] == 0 and call(vm, ns=0, cov=None)[0] == 0
        assert refused("kernel", m=empty, robust_kernel=4) and refused("array", m=empty, sx=None)
        if other != 0:                                               # device arrays that live where the map does not
            far = [torch.from_numpy(v).to(f"cuda:{other}") for v in keep]
            torch.cuda.synchronize(other)
            assert refused("device", sx=C.c_void_p(far[0].data_ptr()), cov=C.c_void_p(far[3].data_ptr()), on_device=1)
    torch.cuda.set_device(0)


def test_nobody_corresponds_on_the_device(gpu):
    """linearize_vgicp against an empty map with torch tensors: the correspondences come back as a device tensor of -1 (the
    fill runs on the device), the sums are zero."""
    import torch
    c = VC.designed(300, (1, 2, 3, 4, 5, 8))
    s = [torch.from_numpy(np.array(v, dtype=F32)).cuda() for v in c]
    cov = torch.eye(3, dtype=torch.float32, device=s[0].device).repeat(s[0].numel(), 1, 1)
    e = tuple(np.zeros(0, dtype=F32) for _ in range(3))
    with gpu.VoxelMap(*e, resolution=VC.EDGE) as empty:
        out = gpu.linearize_vgicp(*s, cov, voxel_map=empty, return_correspondences=True)
        st = gpu.register_last_stats()
    corr = out["corr"]
    assert torch.is_tensor(corr) and corr.device == s[0].device and corr.dtype == torch.int32 and corr.shape == (s[0].numel(),)
    assert bool((corr == -1).all())
    assert out["num_inliers"] == 0 and out["error"] == 0.0 and not out["H"].any() and not out["H_upper"].any() and not out["b"].any()
    assert st["linearizations"] == 0
