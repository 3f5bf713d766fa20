"""fdm_cloud_radius_outlier_removal and fdm_cloud_crop through the Python interface against tests/filter_restate.py, with
host arrays and with device tensors.  The cases and their answers are tests/filter_cases.py's
(tests/test_filter_restate.py checks on the CPU that the two restatements agree and that every case is ADMITTED).

Radius outlier removal, for every case: the counts (count mode) and the masks (both modes) equal the restatement's
exactly, mask mode equals counts >= min_neighbors, the stats add up, a second call gives the same bytes.  The refused
inputs return FDM_ERR_INVALID with poisoned outputs untouched.  The one large case (610 000 points, the sort's large
tile) is held to the counts its construction gives.  The crops: every kind in both modes on one 1 000-point cloud, masks
compared exactly."""
import ctypes as C

import numpy as np
import pytest

import filter_cases as FC
import filter_restate as FR

pytestmark = pytest.mark.gpu
F = np.float32
WHERE = ("host", "device")
MAX_TESTS = 150_000_000_000  # filter::kMaxTests (fdm_filter_host.hpp)


@pytest.fixture(scope="module")
def fdm():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import fastdem_amd
    fastdem_amd.capi.load()
    return fastdem_amd


def placed(cloud, where):
    if where == "host":
        return cloud
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in cloud)


def as_numpy(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def check_against_counts(fdm, name, where, cloud, radius, min_neighbors, want):
    """Both modes against the counts `want`; the stats of both calls."""
    n = want.size
    dev = placed(cloud, where)
    keep_c, counts = fdm.radius_outlier_removal(*dev, radius, min_neighbors, return_counts=True)
    st_c = fdm.ror_last_stats()
    keep_m = fdm.radius_outlier_removal(*dev, radius, min_neighbors)
    st_m = fdm.ror_last_stats()
    print(name, where, "count mode", st_c, "mask mode", st_m)
    counts = as_numpy(counts).astype(np.uint32)
    keep_c, keep_m = as_numpy(keep_c).astype(bool), as_numpy(keep_m).astype(bool)
    assert counts.size == keep_c.size == keep_m.size == n
    assert np.array_equal(counts, want)
    assert np.array_equal(keep_c, want >= min_neighbors)
    assert np.array_equal(keep_m, keep_c)  # mask mode == counts >= min_neighbors from count mode
    for st in (st_c, st_m):
        assert st["n_points"] == n and st["n_kept"] == int(keep_c.sum())
        if n:
            assert st["range"] == 1 and st["candidate_tests"] <= n * (n - 1)
    assert st_c["candidate_tests"] == st_m["candidate_tests"]
    assert st_c["tests_done"] == st_c["candidate_tests"] >= st_m["tests_done"]
    if min_neighbors == 0:
        assert st_m["tests_done"] == 0 and keep_m.all()
    return st_c, st_m


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_counts_and_masks_are_the_restatements(fdm, name, where):
    cloud, radius, min_neighbors = FC.cases()[name]
    st_c, st_m = check_against_counts(fdm, name, where, cloud, radius, min_neighbors, FC.counts(name))
    assert st_c["candidate_tests"] == FR.candidate_tests(FC._pts(cloud), radius)
    if name in FC.KEY_BITS:  # keys wider than 32 bits: k_cluster_keys, the bisections, five radix passes
        assert st_c["key_bits"] == FC.KEY_BITS[name]
    if name == "dense_voxel":
        # own row first, stop at min_neighbors: the 5 000 dense lanes end after a handful of tests, the two outliers walk
        # their whole neighbourhood
        assert st_c["tests_done"] == 5002 * 5001
        assert 2 * 5001 <= st_m["tests_done"] <= 2 * 5001 + 5000 * 16


@pytest.mark.parametrize("where", WHERE)
def test_large_cloud_gives_the_constructed_counts(fdm, where):
    cloud, want = FC.large()
    st_c, _ = check_against_counts(fdm, "large", where, cloud, FC.RADIUS, 5, want)
    assert st_c["candidate_tests"] < 100_000_000  # far below the work bound


@pytest.mark.parametrize("name", ["mixed_r05", "dense_voxel", "line4097", "wide_33_bits", "n2_duplicate"])
def test_two_calls_give_identical_bytes(fdm, name):
    cloud, radius, min_neighbors = FC.cases()[name]
    dev = placed(cloud, "device")
    a = fdm.radius_outlier_removal(*dev, radius, min_neighbors, return_counts=True)
    b = fdm.radius_outlier_removal(*dev, radius, min_neighbors, return_counts=True)
    m1, m2 = fdm.radius_outlier_removal(*dev, radius, min_neighbors), fdm.radius_outlier_removal(*dev, radius, min_neighbors)
    for u, v in ((a[0], b[0]), (a[1], b[1]), (m1, m2), (m1, a[0])):
        assert as_numpy(u).tobytes() == as_numpy(v).tobytes()


def test_empty_cloud(fdm):
    lib = fdm.capi.load()
    n_kept = C.c_uint64(7)
    assert lib.fdm_cloud_radius_outlier_removal(0, None, None, None, 0, 0.5, 3, 0, None, None, C.byref(n_kept)) == 0
    assert n_kept.value == 0
    n_kept = C.c_uint64(7)
    cfg = fdm.capi.FdmCropConfig(0, 0)
    assert lib.fdm_cloud_crop(0, None, None, None, 1, C.byref(cfg), 0, None, C.byref(n_kept)) == 0 and n_kept.value == 0
    import torch
    e = torch.zeros(0, dtype=torch.float32, device="cuda")
    keep, counts = fdm.radius_outlier_removal(e, e, e, 0.5, 1, return_counts=True)
    assert keep.numel() == 0 and counts.numel() == 0 and fdm.remove_invalid(e, e, e).numel() == 0


def poisoned(where, n):
    """(keep, counts, their pointers, a reader): outputs filled with a pattern a refused call must leave alone."""
    if where == "host":
        keep, counts = np.full(n, 0xAB, dtype=np.uint8), np.full(n, 0xDEADBEEF, dtype=np.uint32)
        return keep, counts, [v.ctypes.data_as(C.c_void_p) for v in (keep, counts)]
    import torch
    keep = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
    counts = torch.full((n,), 0x5EADBEEF, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return keep, counts, [C.c_void_p(v.data_ptr()) for v in (keep, counts)]


def untouched(keep, counts):
    k, c = as_numpy(keep), as_numpy(counts)
    return bool((k == 0xAB).all() and (c == c[0]).all() and int(c[0]) & 0xFFFF == 0xBEEF)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(FC.errors()))
def test_undefined_inputs_are_refused(fdm, name, where):
    cloud, radius, word = FC.errors()[name]
    lib = fdm.capi.load()
    n = cloud[0].size
    dev = placed(cloud, where)
    src = [v.ctypes.data_as(C.c_void_p) for v in dev] if where == "host" else [C.c_void_p(v.data_ptr()) for v in dev]
    for with_counts in (True, False):
        keep, counts, out = poisoned(where, n)
        n_kept = C.c_uint64(7)
        rc = lib.fdm_cloud_radius_outlier_removal(n, *src, int(where == "device"), radius, 5, 0, out[0],
                                                  out[1] if with_counts else None, C.byref(n_kept))
        assert rc == -1, (rc, lib.fdm_last_error())  # FDM_ERR_INVALID
        assert word in lib.fdm_last_error().decode() and n_kept.value == 0
        assert untouched(keep, counts), "a refused call wrote to an output"
    with pytest.raises(fdm.EngineError, match=word):
        fdm.radius_outlier_removal(*dev, radius, 5)
    # what the user calls first
    if word == "finite":
        ok = as_numpy(fdm.remove_invalid(*dev)).astype(bool)
        assert int(ok.sum()) == n - 1
        kept = tuple(np.ascontiguousarray(v[ok]) for v in cloud)
        assert fdm.radius_outlier_removal(*kept, radius, 5).size == n - 1


def test_work_bound_refuses_before_the_count_kernel(fdm):
    """560 000 points in one voxel are 3.1e11 candidate tests, above the bound of 1.5e11: refused after the sort and the
    candidate pass, in both modes, outputs untouched."""
    import torch
    lib = fdm.capi.load()
    n = 560000
    v = (torch.arange(n, device="cuda", dtype=torch.float32) % 448.0) / 1024.0  # the lattice of 2^-10 inside [0, 0.4375]
    p = C.c_void_p(v.data_ptr())
    for with_counts in (True, False):
        keep, counts, out = poisoned("device", n)
        n_kept = C.c_uint64(7)
        rc = lib.fdm_cloud_radius_outlier_removal(n, p, p, p, 1, 0.5, 5, 0, out[0], out[1] if with_counts else None,
                                                  C.byref(n_kept))
        assert rc == -1 and b"candidate tests" in lib.fdm_last_error() and n_kept.value == 0
        st = fdm.ror_last_stats()
        assert st["candidate_tests"] == n * (n - 1) > MAX_TESTS and st["tests_done"] == 0
        assert untouched(keep, counts)


# ------------------------------------------------------------------ the crops ----
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(FC.crop_cases()))
def test_crop_masks_are_the_restatements(fdm, name, where):
    fn, args, want = FC.crop_cases()[name]
    dev = placed(FC.crop_cloud(), where)
    for mode, mask in want.items():
        kw = {} if name == "finite" else {"mode": mode}
        got = getattr(fdm, fn)(*dev, *args, **kw)
        again = getattr(fdm, fn)(*dev, *args, **kw)
        if where == "host":
            assert got.dtype == bool
        else:
            import torch
            assert got.dtype == torch.uint8 and got.is_cuda
        got = as_numpy(got).astype(bool)
        print(name, where, mode, "kept", int(got.sum()), "of", got.size)
        assert np.array_equal(got, mask), np.nonzero(got != mask)[0][:10]
        assert as_numpy(again).astype(bool).tobytes() == got.tobytes()


def test_crop_past_the_grids_edge(fdm):
    """n = 262 145: k_filter_keep's grid is capped at 1024 blocks of 256, the last point is the strided loop's first."""
    import torch
    n = FC.GRID_EDGE
    rng = np.random.default_rng(n)
    x, y, z = (rng.normal(0.0, 3.0, n).astype(F) for _ in range(3))
    x[-1], y[-1], z[-1] = 3.0, 4.0, 0.0      # exactly on the outer sphere: kept, by the loop's second round
    x[-2], y[-2], z[-2] = np.nan, 0.0, 0.0
    want = FR.crop_range(x, y, z, 1.0, 5.0, "inside")
    assert want[-1] and not want[-2] and want.any() and not want.all()
    for where in WHERE:
        got = as_numpy(fdm.crop_range(*placed((x, y, z), where), 1.0, 5.0)).astype(bool)
        assert np.array_equal(got, want)
    assert np.array_equal(as_numpy(fdm.remove_invalid(*placed((x, y, z), "device"))).astype(bool), FR.remove_invalid(x, y, z))
    assert torch.cuda.is_available()
