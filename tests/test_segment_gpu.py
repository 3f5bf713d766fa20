"""fdm_cloud_segment_ground, fdm_cloud_segment_plane and fdm_cloud_segment_planes through the Python interface against
tests/seg_restate.py, with host arrays and with device tensors.  The cases and the restatement's answers are
tests/seg_cases.py's (tests/test_seg_restate.py checks on the CPU that every plane case is ADMITTED: its refined
coefficients and inliers do not depend on the summation order or the eigen-solver).

Ground: both lists bit for bit; the undefined inputs return FDM_ERR_INVALID with the lists untouched.  Plane: iterations,
success and the inlier count; the unrefined model's bits (refine_model off); the refined coefficients' bits and the inlier
list; independently of any admission, the returned inliers are what the restatement's collect gives for the engine's OWN
coefficients; fitness = n_inliers / n_indices exactly; the batches launched.

The large cases (tests/seg_cases_large.py: lists past the scoring kernel's grid, the refinement's summation grid, the
index check's grid, the scan's carry and the sort's tile switch) are held to the same assertions."""
import ctypes as C

import numpy as np
import pytest

import seg_cases as SC
import seg_cases_large as SL
import seg_restate as SR

pytestmark = pytest.mark.gpu
F = np.float32
WHERE = ("host", "device")


@pytest.fixture(scope="module")
def fdm():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import fastdem_amd
    fastdem_amd.capi.load()
    return fastdem_amd


def placed(cloud, where, indices=None):
    """The cloud (and an index list) as numpy arrays or as device tensors."""
    if where == "host":
        return cloud, indices
    import torch
    dev = tuple(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in cloud)
    return dev, None if indices is None else torch.from_numpy(indices.astype(np.int64)).cuda()


def as_numpy(a):
    return a.cpu().numpy().astype(np.uint32) if hasattr(a, "cpu") else np.asarray(a, dtype=np.uint32)


def bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


# ------------------------------------------------------------------ ground ----
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(SC.ground_cases()))
def test_ground_lists_are_the_restatements(fdm, name, where):
    cloud, kw = SC.ground_cases()[name]
    want_g, want_o = SC.ground_answer(name)
    dev, _ = placed(cloud, where)
    g, o = fdm.segment_ground(*dev, **kw)
    g, o = as_numpy(g), as_numpy(o)
    assert g.size == want_g.size and o.size == want_o.size, (g.size, want_g.size, o.size, want_o.size)
    assert np.array_equal(g, want_g) and np.array_equal(o, want_o)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(SL.ground_cases()))
def test_ground_600k_lists_are_the_restatements(fdm, name, where):
    cloud, kw = SL.ground_cases()[name]
    want_g, want_o = SL.ground_answer(name)
    dev, _ = placed(cloud, where)
    g, o = fdm.segment_ground(*dev, **kw)
    g, o = as_numpy(g), as_numpy(o)
    assert g.size == want_g.size and o.size == want_o.size, (g.size, want_g.size, o.size, want_o.size)
    assert np.array_equal(g, want_g) and np.array_equal(o, want_o)


def test_ground_empty_cloud_and_null_lists(fdm):
    e = np.zeros(0, dtype=F)
    g, o = fdm.segment_ground(e, e, e)
    assert g.size == 0 and o.size == 0
    # either list may be NULL: the counts still come back
    lib = fdm.capi.load()
    (x, y, z), _ = SC.ground_cases()["n255_edges"]
    want_g, want_o = SC.ground_answer("n255_edges")
    ng, no = C.c_uint64(7), C.c_uint64(7)
    only = np.zeros(x.size, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.fdm_cloud_segment_ground(x.size, ptr(x), ptr(y), ptr(z), 0, None, 0, None, ptr(only), C.byref(ng),
                                        C.byref(no)) == 0
    assert (ng.value, no.value) == (want_g.size, want_o.size) and np.array_equal(only[:no.value], want_o)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(SC.ground_errors()))
def test_ground_undefined_inputs_are_refused(fdm, name, where):
    cloud, kw = SC.ground_errors()[name]
    lib = fdm.capi.load()
    n = cloud[0].size
    cfg = fdm.capi.FdmGroundSegConfig(kw.get("grid_resolution", 0.5), kw.get("cell_percentile", 0.2), 0.3, 0.5, 2)
    ng, no = C.c_uint64(0), C.c_uint64(0)
    if where == "host":
        lists = [np.full(n, 0xDEADBEEF, dtype=np.uint32) for _ in range(2)]
        ptrs = [v.ctypes.data_as(C.c_void_p) for v in (*cloud, *lists)]
    else:
        import torch
        dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in cloud]
        lists = [torch.full((n,), 0x5EADBEEF, dtype=torch.int32, device="cuda") for _ in range(2)]
        ptrs = [C.c_void_p(v.data_ptr()) for v in (*dev, *lists)]
        torch.cuda.synchronize()
    rc = lib.fdm_cloud_segment_ground(n, ptrs[0], ptrs[1], ptrs[2], int(where == "device"), C.byref(cfg), 0, ptrs[3],
                                      ptrs[4], C.byref(ng), C.byref(no))
    assert rc == -1, (rc, lib.fdm_last_error())  # FDM_ERR_INVALID
    assert (ng.value, no.value) == (0, 0)
    for v in lists:
        host = v.cpu().numpy() if where == "device" else v
        assert (host == host[0]).all() and int(host[0]) & 0xFFFF == 0xBEEF, "a refused call wrote to a list"
    with pytest.raises(fdm.EngineError):
        fdm.segment_ground(*cloud, **kw)


# ------------------------------------------------------------------ planes ----
def check_against_restatement(r, want, cloud, kw, n_list):
    inl = as_numpy(r.inliers)
    assert (r.iterations, r.success, inl.size) == (want["iterations"], want["success"], want["inliers"].size)
    assert np.array_equal(bits(r.coefficients), bits(want["coefficients"])), (r.coefficients, want["coefficients"])
    assert np.array_equal(inl, want["inliers"])
    assert r.fitness == (inl.size / float(n_list) if want["iterations"] else 0.0)
    if want["iterations"]:  # independently of any admission: the inliers of the engine's own coefficients
        idx = kw.get("indices")
        idx = np.arange(cloud[0].size, dtype=np.uint32) if idx is None else idx
        own = SR.collect(*cloud, idx, np.asarray(r.coefficients, dtype=F), F(kw["distance_threshold"]))
        assert np.array_equal(inl, own)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(SC.plane_cases()))
def test_plane_is_the_restatements(fdm, name, where):
    cloud, kw = SC.plane_cases()[name]
    want = SC.plane_answer(name)
    idx = kw.get("indices")
    n_list = cloud[0].size if idx is None else idx.size
    dev, dev_idx = placed(cloud, where, idx)
    args = {k: v for k, v in kw.items() if k != "indices"}
    r = fdm.segment_plane(*dev, indices=dev_idx, **args)
    check_against_restatement(r, want, cloud, kw, n_list)
    if kw.get("refine_model", True) is False:
        assert np.array_equal(bits(r.coefficients), bits(want["unrefined"]))
    st = fdm.segment_last_stats()
    B = st["batch"] if n_list >= 3 else SC.BATCH
    assert B == SC.BATCH
    passes = want.get("loop_iterations", 0)
    assert st["n_batches"] >= -(-passes // B) and st["n_invalid_samples"] == want["valid"].count(0)
    if name in SC.WITHIN_ONE_BATCH:
        assert st["n_batches"] == 1
    if name in SC.ACROSS_BATCH_EDGES:
        assert st["n_batches"] >= 3
    if name in SC.AT_THE_CAP:
        assert st["n_hypotheses"] == passes == kw.get("max_iterations", 1000)  # the last batch is cut to the cap


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(SL.plane_cases()))
def test_large_plane_is_the_restatements(fdm, name, where):
    cloud, kw = SL.plane_cases()[name]
    want = SL.plane_answer(name)
    idx = kw.get("indices")
    n_list = cloud[0].size if idx is None else idx.size
    dev, dev_idx = placed(cloud, where, idx)
    r = fdm.segment_plane(*dev, indices=dev_idx, **{k: v for k, v in kw.items() if k != "indices"})
    check_against_restatement(r, want, cloud, kw, n_list)
    st = fdm.segment_last_stats()
    passes = want["loop_iterations"]
    assert st["batch"] == SC.BATCH and st["n_batches"] == 1 and st["n_invalid_samples"] == want["valid"].count(0)
    assert st["n_hypotheses"] == (passes if name in SL.count_cases() else SC.BATCH)
    if name in SL.count_cases():  # run to the cap: one batch of 128, both halves of k_plane_count
        assert passes == kw["max_iterations"] == SC.BATCH and n_list > SL.PLANE_COUNT_SWEEP
    else:
        assert as_numpy(r.inliers).size > SL.PLANE_SUM_SWEEP


@pytest.mark.parametrize("name", sorted(SL.sum_cases()))
def test_plane_two_calls_give_identical_bits(fdm, name):
    """The refinement's sums are a fixed tree over a grid that depends on the inlier count alone: past 65 536 inliers,
    where a lane takes several terms, a repeated call still gives the same bits."""
    cloud, kw = SL.sum_cases()[name]
    dev, _ = placed(cloud, "device")
    a, b = fdm.segment_plane(*dev, **kw), fdm.segment_plane(*dev, **kw)
    assert bits(a.coefficients).tobytes() == bits(b.coefficients).tobytes()
    assert as_numpy(a.inliers).tobytes() == as_numpy(b.inliers).tobytes()
    assert (a.iterations, a.fitness, a.success) == (b.iterations, b.fitness, b.success)


def test_plane_result_does_not_depend_on_the_batch(fdm):
    lib = fdm.capi.load()
    cloud, kw = SC.plane_cases()["scene20"]
    want = SC.plane_answer("scene20")
    try:
        for batch in (1, 32, 64):
            assert lib.fdm_segment_debug_batch(batch) == 0
            if batch == 1:  # (one launch per pass: a short loop is enough)
                r = fdm.segment_plane(*cloud, max_iterations=40, **kw)
                w = SR.segment_plane(*cloud, max_iterations=40, **kw)
                assert fdm.segment_last_stats()["n_batches"] == 40
            else:
                r, w = fdm.segment_plane(*cloud, **kw), want
            assert fdm.segment_last_stats()["batch"] == batch
            check_against_restatement(r, w, cloud, kw, cloud[0].size)
    finally:
        lib.fdm_segment_debug_batch(0)
    assert lib.fdm_segment_debug_batch(129) == -1 and lib.fdm_segment_debug_batch(-1) == -1


@pytest.mark.parametrize("where", WHERE)
def test_plane_index_out_of_range_is_refused(fdm, where):
    cloud, kw = SC.INDEX_ERROR
    dev, dev_idx = placed(cloud, where, kw["indices"])
    with pytest.raises(fdm.EngineError, match="index"):
        fdm.segment_plane(*dev, distance_threshold=kw["distance_threshold"], indices=dev_idx)


@pytest.mark.parametrize("where", WHERE)
def test_plane_index_past_the_check_grid_is_refused(fdm, where):
    """524 289 entries whose only bad one is the last: k_seg_index_check's grid is capped at 2048 blocks of 256, so that
    entry is seen by the strided loop alone.  Refused, the inlier list and the result untouched."""
    cloud, kw = SC.INDEX_ERROR
    idx = SL.index_check_stride(cloud[0].size)
    lib = fdm.capi.load()
    cfg = fdm.capi.FdmRansacConfig(float(F(kw["distance_threshold"])), 1000, 0.99, 3, 1)
    res = fdm.capi.FdmRansacResult()
    if where == "host":
        inl = np.full(idx.size, 0xDEADBEEF, dtype=np.uint32)
        ptrs = [v.ctypes.data_as(C.c_void_p) for v in (*cloud, idx, inl)]
    else:
        import torch
        dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in cloud]
        d_idx = torch.from_numpy(idx.astype(np.int64)).to(torch.int32).cuda()
        inl = torch.full((idx.size,), 0x5EADBEEF, dtype=torch.int32, device="cuda")
        ptrs = [C.c_void_p(v.data_ptr()) for v in (*dev, d_idx, inl)]
        torch.cuda.synchronize()
    rc = lib.fdm_cloud_segment_plane(cloud[0].size, ptrs[0], ptrs[1], ptrs[2], int(where == "device"), ptrs[3], idx.size,
                                     C.byref(cfg), 0, ptrs[4], C.byref(res))
    assert rc == -1 and b"index" in lib.fdm_last_error(), (rc, lib.fdm_last_error())  # FDM_ERR_INVALID
    host = inl.cpu().numpy() if where == "device" else inl
    assert (host == host[0]).all() and int(host[0]) & 0xFFFF == 0xBEEF, "a refused call wrote to the inlier list"
    assert (res.iterations, res.success, res.n_inliers, res.fitness) == (0, 0, 0, 0.0)
    assert list(res.coefficients) == [0.0, 0.0, 1.0, 0.0]
    dev, dev_idx = placed(cloud, where, idx)
    with pytest.raises(fdm.EngineError, match="index"):
        fdm.segment_plane(*dev, distance_threshold=kw["distance_threshold"], indices=dev_idx)
    # the same list without its last entry is taken
    dev, dev_idx = placed(cloud, where, idx[:-1])
    r = fdm.segment_plane(*dev, distance_threshold=kw["distance_threshold"], indices=dev_idx, max_iterations=8)
    want = SR.segment_plane(*cloud, distance_threshold=kw["distance_threshold"], indices=idx[:-1], max_iterations=8)
    assert (r.iterations, r.success) == (want["iterations"], want["success"]) == (8, True)


def test_plane_outliers_complete_the_inliers(fdm):
    cloud, kw = SC.plane_cases()["scene45"]
    for where in WHERE:
        dev, _ = placed(cloud, where)
        r = fdm.segment_plane(*dev, **kw)
        out = as_numpy(r.outliers(cloud[0].size))
        assert np.array_equal(out, SR.outliers(SC.plane_answer("scene45")["inliers"], cloud[0].size))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(SC.multi_cases()))
def test_multiple_planes_are_the_restatements(fdm, name, where):
    cloud, kw = SC.multi_cases()[name]
    want = SC.multi_answer(name)
    dev, _ = placed(cloud, where)
    res = fdm.segment_multiple_planes(*dev, **kw)
    assert len(res) == len(want)
    remaining = cloud[0].size
    for r, w in zip(res, want):
        inl = as_numpy(r.inliers)
        assert (r.iterations, r.success) == (w["iterations"], w["success"])
        assert np.array_equal(bits(r.coefficients), bits(w["coefficients"]))
        assert np.array_equal(inl, w["inliers"])
        assert r.fitness == inl.size / float(remaining)
        remaining -= inl.size
    got = np.concatenate([as_numpy(r.inliers) for r in res]) if res else np.zeros(0, dtype=np.uint32)
    assert np.unique(got).size == got.size, "a point was given to two planes"


def test_multiple_planes_limits(fdm):
    cloud, kw = SC.multi_cases()["two_planes"]
    one = fdm.segment_multiple_planes(*cloud, **{**kw, "max_planes": 1})
    assert len(one) == 1 and np.array_equal(as_numpy(one[0].inliers), SC.multi_answer("two_planes")[0]["inliers"])
    assert fdm.segment_multiple_planes(*cloud, **{**kw, "min_fitness": 0.9}) == []
    assert fdm.segment_multiple_planes(*cloud, **{**kw, "max_planes": 0}) == []
    two = SC._xyz([(0, 0, 0), (1, 0, 0)])
    assert fdm.segment_multiple_planes(*two) == []
