"""Normal and covariance estimation on the device (fastdem_amd/csrc/fdm_normals.hpp, fdm_cloud_estimate_normals) against
the brute-force NumPy restatement of nanoPCL's k-NN estimators (tests/normal_restate.py): normals, cov9, n_invalid and
the invalid pattern bit for bit — both sides take the neighbours by (d2, input index), the sums in that order and the
solver's trig correctly rounded.  The clouds are tests/normal_cases.py's; which path of the search each reaches is proven
on the CPU in tests/test_normal_restate.py and read back here from the stats.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

import normal_cases as NC
import normal_restate as NR

pytestmark = pytest.mark.gpu
F32 = np.float32
ORIGIN = (0.0, 0.0, 0.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def call(gpu, x, y, z, k, viewpoint=ORIGIN, form="both", on_device=False, partial=False):
    """(rc, normals[n, 3] or None, cov[n, 3, 3] indexed [row][column] or None, n_invalid) of fdm_cloud_estimate_normals
    through the C ABI.  form: "normals", "cov" or "both".  Outputs are pre-filled with 7 to show what was written."""
    lib = gpu.capi.load()
    n = x.size
    vp = (C.c_float * 3)(*viewpoint)
    bad = C.c_uint64(123)
    soa = np.full((3, max(n, 1)), 7, dtype=F32)
    cov9 = np.full((max(n, 1), 9), 7, dtype=F32)
    want_n, want_c = form in ("normals", "both"), form in ("cov", "both")
    if on_device:
        import torch
        keep = [torch.from_numpy(np.array(v, dtype=F32)).cuda() for v in (x, y, z, soa, cov9)]   # (copies: the cases are read-only)
        px, py, pz = (C.c_void_p(t.data_ptr()) for t in keep[:3])
        pn = [C.c_void_p(keep[3][a].data_ptr()) for a in range(3)]
        pc = C.c_void_p(keep[4].data_ptr())
    else:
        keep = [np.ascontiguousarray(v, dtype=F32) for v in (x, y, z)]
        px, py, pz = (v.ctypes.data_as(C.c_void_p) for v in keep)
        pn = [soa[a].ctypes.data_as(C.c_void_p) for a in range(3)]
        pc = cov9.ctypes.data_as(C.c_void_p)
    if not want_n:
        pn = [None, None, None]
    if partial:
        pn[1] = None
    rc = lib.fdm_cloud_estimate_normals(n, px, py, pz, int(on_device), int(k), vp, 0, pn[0], pn[1], pn[2],
                                        pc if want_c else None, C.byref(bad))
    if on_device:
        import torch
        torch.cuda.synchronize()
        soa, cov9 = keep[3].cpu().numpy(), keep[4].cpu().numpy()
    normals = np.ascontiguousarray(soa[:, :n].T)
    cov = np.ascontiguousarray(cov9[:n].reshape(n, 3, 3).transpose(0, 2, 1))
    return rc, normals, cov, int(bad.value)


def check(gpu, name, k, viewpoint=ORIGIN, form="both", on_device=False):
    (x, y, z), rows, normals, cov, invalid = NC.restated(name, k, viewpoint)
    rc, got_n, got_c, got_bad = call(gpu, x, y, z, k, viewpoint, form, on_device)
    assert rc == 0, gpu.capi.load().fdm_last_error()
    st = gpu.normals_last_stats()
    sel = slice(None) if rows is None else rows
    if form in ("normals", "both"):
        diff = np.flatnonzero((bits(got_n[sel]) != bits(normals)).any(axis=1))
        assert diff.size == 0, f"{name} k={k}: {diff.size} normals differ, e.g. row {diff[0]}: {got_n[sel][diff[0]]!r} vs {normals[diff[0]]!r}"
        assert np.array_equal(~got_n[sel].any(axis=1), invalid)     # a valid normal has unit length, an invalid one is zero
    else:
        assert (got_n == 7).all()                                    # not asked for, not touched
    if form in ("cov", "both"):
        diff = np.flatnonzero((bits(got_c[sel]) != bits(cov)).reshape(-1, 9).any(axis=1))
        assert diff.size == 0, f"{name} k={k}: {diff.size} covariances differ, e.g. row {diff[0]}:\n{got_c[sel][diff[0]]!r} vs\n{cov[diff[0]]!r}"
    else:
        assert (got_c == 7).all()
    if rows is None:
        assert got_bad == int(invalid.sum()) == st["n_invalid"], (got_bad, int(invalid.sum()), st)
    assert st["n_queries"] == x.size and 0 <= st["n_fallback"] <= x.size
    print(f"{name} k={k} {form} {'device' if on_device else 'host'}: grid {st['grid_x']} x {st['grid_y']} of {st['voxel']:.4g}, "
          f"{st['n_fallback']} queued, {st['n_invalid']} invalid")
    return st


# ---- bucket edges: KB = 4, 16, 32, 64 at both ends, in the search lanes and (isolated) in the queue ----
@pytest.mark.parametrize("k", [3, 4, 5, 16, 17, 20, 32, 33, 64])
def test_bucket_edges(gpu, k):
    st = check(gpu, "surface", k)
    assert st["grid_x"] > 2 * NC.SHELLS + 1 and st["grid_y"] > 2 * NC.SHELLS + 1   # the rings' stopping rule decides


@pytest.mark.parametrize("k", [3, 4, 5, 16, 17, 20, 32, 33, 64])
def test_fallback_queue(gpu, k):
    st = check(gpu, "isolated", k)
    assert st["n_fallback"] >= NC.must_queue("isolated", k) >= 1, st   # the far points the rings cannot settle


@pytest.mark.parametrize("form", ["normals", "cov", "both"])
@pytest.mark.parametrize("on_device", [False, True])
def test_forms_on_host_and_device_arrays(gpu, form, on_device):
    check(gpu, "surface", 20, (1.0, -2.0, 30.0), form, on_device)
    check(gpu, "isolated", 20, (1.0, -2.0, 30.0), form, on_device)   # ... and through the queue kernel


# ---- k against n ----
@pytest.mark.parametrize("n", [1, 2, 3, 5, 10, 255, 256, 257])
@pytest.mark.parametrize("k", [10, -1])
def test_k_against_n(gpu, n, k):
    name = f"n{n}"
    x, y, z = NC.cloud(name)
    if k < 0 and n > 64:                                             # "every point" is more than 64
        rc, _, _, bad = call(gpu, x, y, z, k)
        assert rc == gpu.capi.FDM_ERR_INVALID and bad == 0
        return
    st = check(gpu, name, k)
    if n < 3:
        assert st["n_invalid"] == n


def test_empty_cloud_touches_nothing(gpu):
    e = np.zeros(0, dtype=F32)
    rc, n, c, bad = call(gpu, e, e, e, 10)
    assert rc == 0 and bad == 0 and n.shape == (0, 3)
    lib = gpu.capi.load()
    out = np.full(4, 7, dtype=F32)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.fdm_cloud_estimate_normals(0, None, None, None, 0, 10, None, 0, p, p, p, None, None) == 0
    assert (out == 7).all()
    normals = gpu.estimate_normals(e, e, e)
    assert normals.shape == (0, 3)


# ---- refusals ----
def test_refusals(gpu):
    x, y, z = NC.cloud("n257")
    INVALID = gpu.capi.FDM_ERR_INVALID
    assert call(gpu, x, y, z, 65)[0] == INVALID                      # effective_k = 65
    assert call(gpu, x[:65], y[:65], z[:65], 65)[0] == INVALID       # n = 65: still 65
    assert call(gpu, x[:64], y[:64], z[:64], 65)[0] == 0             # min(65, 64) = 64: served
    assert call(gpu, x, y, z, 10, partial=True)[0] == INVALID        # nx and nz without ny
    assert call(gpu, x, y, z, 10, form="none")[0] == INVALID         # nothing to estimate
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            c = [x.copy(), y.copy(), z.copy()]
            c[axis][200] = bad
            assert call(gpu, *c, 10)[0] == INVALID
    with pytest.raises(gpu.EngineError):
        gpu.estimate_normals(x, y, z, 65)


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("on_device", [False, True])
def test_fewer_than_three_neighbours_is_all_invalid_not_an_error(gpu, k, on_device):
    x, y, z = NC.cloud("n257")
    rc, n, c, bad = call(gpu, x, y, z, k, on_device=on_device)
    assert rc == 0 and bad == 257
    assert not n.any() and np.array_equal(c, np.tile(np.eye(3, dtype=F32), (257, 1, 1)))
    assert gpu.normals_last_stats()["n_invalid"] == 257


# ---- the whole-cloud exit, degenerate input, ties ----
def test_whole_cloud_exit(gpu):
    for k in (10, 20):
        st = check(gpu, "small_grid", k)
        assert st["n_fallback"] == 0 and st["grid_x"] <= NC.SHELLS + 1 and st["grid_y"] <= NC.SHELLS + 1, st


def test_identical_points_are_all_invalid(gpu):
    st = check(gpu, "identical", 10)
    assert st["n_invalid"] == 100 and (st["grid_x"], st["grid_y"]) == (1, 1)
    rc, n, c, bad = call(gpu, *NC.cloud("identical"), 10)
    assert bad == 100 and not n.any() and np.array_equal(c, np.tile(np.eye(3, dtype=F32), (100, 1, 1)))


def test_collinear_points(gpu):
    check(gpu, "collinear", 5)


def test_duplicates_of_the_query_at_lower_and_higher_indices(gpu):
    check(gpu, "duplicates", 10)
    check(gpu, "duplicates", 3)                                      # three of the five copies are all the neighbours


@pytest.mark.parametrize("name", ["xy5", "xy10", "xz5", "xz10", "tilted5", "tilted10"])
def test_lattice_ties(gpu, name):
    """Equal distances everywhere: both sides break them by input index.  The reference's own expectations of these
    lattices (test_geometry.cpp) are checked on what the device returned."""
    check(gpu, name, 10)
    x, y, z = NC.cloud(name)
    _, n, c, bad = call(gpu, x, y, z, 10)
    assert bad == 0
    if name.startswith("tilted"):
        e = np.array([-0.5, -0.3, 1.0]) / np.sqrt(0.25 + 0.09 + 1.0)
        assert (np.abs(np.abs(n.astype(np.float64) @ e) - 1.0) < 0.1).all()
    else:
        axis = 2 if name.startswith("xy") else 1
        assert (np.abs(np.abs(n[:, axis]) - 1.0) < 0.1).all() and (np.abs(np.delete(n, axis, axis=1)) < 0.1).all()
    length = np.sqrt((n.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() < 1e-5
    w = np.linalg.eigvalsh(c.astype(np.float64))
    assert np.abs(w[:, 0] - 1e-3).max() < 1e-4 and np.abs(w[:, 1:] - 1.0).max() < 0.1


@pytest.mark.parametrize("viewpoint", [(2.0, 2.0, 10.0), (2.0, 2.0, -10.0), (2.0, 2.0, 0.0)])
def test_viewpoint_above_below_and_in_the_plane(gpu, viewpoint):
    check(gpu, "xy5", 10, viewpoint)
    _, n, _, _ = call(gpu, *NC.cloud("xy5"), 10, viewpoint)
    if viewpoint[2] != 0:
        assert (np.sign(n[:, 2]) == np.sign(viewpoint[2])).all()
    else:                                                            # a dot of exactly 0: as without a viewpoint rule
        raw = NR.estimate(*NC.cloud("xy5"), 10, None)[0]
        assert np.array_equal(bits(n), bits(raw))


# ---- scale ----
def test_utm_sized_offsets(gpu):
    check(gpu, "utm", 20, (5.0e5, 4.9e5, 150.0))


def test_large_cloud_at_sampled_queries(gpu):
    st = check(gpu, "large", 20, (5.0e5, 4.9e5, 150.0))
    assert st["n_queries"] == 200_000


# ---- the Python entry ----
def test_python_entry_numpy_and_torch(gpu):
    import torch
    (x, y, z), _, normals, cov, invalid = NC.restated("surface", 20, (1.0, -2.0, 30.0))
    n1 = gpu.estimate_normals(x, y, z, 20, (1.0, -2.0, 30.0))
    n2, c2, st = gpu.estimate_normals(x, y, z, 20, (1.0, -2.0, 30.0), covariances=True, return_stats=True)
    assert np.array_equal(bits(n1), bits(normals)) and np.array_equal(bits(n2), bits(normals))
    assert np.array_equal(bits(c2), bits(cov)) and st["n_invalid"] == int(invalid.sum())
    assert st["ms"] == (0.0, 0.0, 0.0, 0.0)                          # no events unless fdm_cloud_debug_profile is on
    d = [torch.from_numpy(np.array(v)).cuda() for v in (x, y, z)]     # (copies: the case arrays are read-only)
    n3, c3 = gpu.estimate_normals(*d, 20, (1.0, -2.0, 30.0), covariances=True)
    assert n3.is_cuda and c3.is_cuda and n3.shape == (x.size, 3) and c3.shape == (x.size, 3, 3)
    assert np.array_equal(bits(n3.cpu().numpy()), bits(normals)) and np.array_equal(bits(c3.cpu().numpy()), bits(cov))
