"""fdm_cloud_cluster through the Python interface against the canonical form of tests/cluster_restate.py's result, with
host arrays and with device tensors.  The cases and their answers are tests/cluster_cases.py's
(tests/test_cluster_restate.py checks on the CPU that every case is ADMITTED and that the restatement's partition is the
brute-force one).

For every case: n_clusters, offsets and cluster_indices equal the canonical form exactly; labels agree with them;
noise_indices is the complement; the stats add up; a second call gives the same bytes.  The refused inputs return
FDM_ERR_INVALID with poisoned outputs untouched.

The large cases (tests/cluster_cases_large.py: lists past the sort's tile switch, the scan's carry and the index
check's grid; one component over a thousand blocks) are held to the same assertions against the canonical form their
construction gives."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as CC
import cluster_cases_large as CL
import cluster_restate as CR

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
    if where == "host":
        return cloud, indices
    import torch
    dev = tuple(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in cloud)
    return dev, None if indices is None else torch.from_numpy(indices.astype(np.int64)).cuda()


def as_numpy(a):
    return a.cpu().numpy().astype(np.uint32) if hasattr(a, "cpu") else np.asarray(a, dtype=np.uint32)


def run(fdm, name, where):
    cloud, kw = (CC.cases() if name in CC.cases() else CL.cases())[name][:2]
    dev, dev_idx = placed(cloud, where, kw.get("indices"))
    args = {k: v for k, v in kw.items() if k != "indices"}
    return fdm.euclidean_cluster(*dev, indices=dev_idx, **args)


def check_canonical_form(fdm, name, where, cloud, kw, answer, n_components):
    want_ind, want_off, want_lab = answer
    idx = kw.get("indices")
    m = cloud[0].size if idx is None else idx.size
    r = run(fdm, name, where)
    st = fdm.cluster_last_stats()
    ind, off, lab = as_numpy(r.indices), as_numpy(r.offsets), as_numpy(r.labels)
    print(name, where, "clusters", r.num_clusters, "points", ind.size, st)
    assert r.num_clusters == want_off.size - 1 and r.total_clustered_points == want_ind.size
    assert np.array_equal(off, want_off)
    assert np.array_equal(ind, want_ind)
    assert lab.size == m and np.array_equal(lab, want_lab)
    # labels against the CSR itself, whatever the answer: position p of cluster k carries k + 1
    entries = np.arange(cloud[0].size, dtype=np.uint32) if idx is None else idx
    pos = np.nonzero(lab)[0]
    order = np.argsort(lab[pos], kind="stable")
    assert np.array_equal(entries[pos[order]], ind)
    assert np.array_equal(np.bincount(lab[pos], minlength=off.size)[1:], np.diff(off.astype(np.int64)))
    assert np.array_equal(as_numpy(r.cluster_sizes()), np.diff(want_off.astype(np.int64)))
    if r.num_clusters:
        assert np.array_equal(as_numpy(r.cluster_indices(0)), want_ind[:want_off[1]])
    assert np.array_equal(as_numpy(r.noise_indices(cloud[0].size)), CR.noise_indices(want_ind, cloud[0].size))
    # the stats
    assert st["n_points"] == m and st["n_kept"] == r.num_clusters and st["n_clustered"] == ind.size
    assert st["n_components"] == st["n_kept"] + st["n_rejected"]
    assert st["unions"] == m - st["n_components"]
    assert st["neighbour_pairs"] <= st["tests"] <= st["candidate_pairs"] <= m * (m - 1) // 2
    assert st["neighbour_pairs"] >= st["unions"]
    if m:
        assert st["n_components"] == n_components and st["range"] == 1
    return st


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(CC.cases()))
def test_clusters_are_the_canonical_form(fdm, name, where):
    cloud, kw = CC.cases()[name]
    st = check_canonical_form(fdm, name, where, cloud, kw, CC.answer(name), CC.n_components(name) if CC.list_length(name) else 0)
    if name in CC.KEY_BITS:  # keys wider than 32 bits: k_cluster_keys, k_cluster_ranges' bisection, 5 .. 8 radix passes
        assert st["key_bits"] == CC.KEY_BITS[name]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(CL.cases()))
def test_large_clusters_are_the_constructed_form(fdm, name, where):
    cloud, kw, _ = CL.cases()[name]
    *answer, n_components = CL.answer(name)
    st = check_canonical_form(fdm, name, where, cloud, kw, tuple(answer), n_components)
    assert st["candidate_pairs"] < 100_000_000  # far below the work bound of 1.5e11


@pytest.mark.parametrize("name", ["mixed70k", "dense_voxel", "singletons_min1", "line4097", "subset_duplicate",
                                  "blobs_688k_min10"])
def test_two_calls_give_identical_bytes(fdm, name):
    a, b = run(fdm, name, "device"), run(fdm, name, "device")
    for u, v in ((a.indices, b.indices), (a.offsets, b.offsets), (a.labels, b.labels)):
        assert as_numpy(u).tobytes() == as_numpy(v).tobytes()


def test_work_bound_refuses_instead_of_running_for_long(fdm):
    """560 000 points in one voxel are 1.57e11 candidate pairs, above the documented bound of 1.5e11 (about a second of
    the merge): refused after the sort and the interval pass, outputs untouched.  548 000 (1.501e11) too, 547 000
    (1.496e11) would run: not run here, it would take that second."""
    import torch
    lib = fdm.capi.load()
    for n in (560000, 548000):
        v = (torch.arange(n, device="cuda", dtype=torch.float32) % 448.0) / 1024.0  # the lattice of 2^-10 inside [0, 0.4375]
        outs = [torch.full((n + 1,), 0x5EADBEEF, dtype=torch.int32, device="cuda") for _ in range(3)]
        count = C.c_uint64(7)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        torch.cuda.synchronize()
        rc = lib.fdm_cloud_cluster(n, p(v), p(v), p(v), 1, None, 0, None, 0, p(outs[0]), p(outs[1]), p(outs[2]), C.byref(count))
        assert rc == -1 and b"candidate pairs" in lib.fdm_last_error() and count.value == 0
        assert fdm.cluster_last_stats()["candidate_pairs"] == n * (n - 1) // 2 > 150_000_000_000
        for t in outs:
            assert bool((t == 0x5EADBEEF).all())


def test_apply_cluster_labels(fdm):
    cloud, _ = CC.cases()["spheres"]
    want_ind, want_off, _ = CC.answer("spheres")
    for where in WHERE:
        r = run(fdm, "spheres", where)
        lab = fdm.apply_cluster_labels(r, cloud[0].size, semantic_class=1)
        assert lab.dtype == np.uint32 and np.array_equal(lab, CR.apply_cluster_labels(want_ind, want_off, cloud[0].size, 1))
        assert int(((lab & 0xFFFF) > 0).sum()) == r.total_clustered_points  # test_segmentation.cpp:249-256
    # more than 65 535 clusters do not fit the instance id: truncated as in the reference (clusters of one point, by hand)
    many = fdm.ClusterResult(np.arange(65537, dtype=np.uint32), np.arange(65538, dtype=np.uint32), None)
    lab = fdm.apply_cluster_labels(many, 65537, semantic_class=3)
    assert np.array_equal(lab, CR.apply_cluster_labels(many.indices, many.offsets, 65537, 3))
    assert lab[65535] == 3 << 16 and lab[65536] == (3 << 16) | 1


def test_empty_list_writes_the_first_offset(fdm):
    lib = fdm.capi.load()
    import torch
    off_h = np.full(1, 0xDEADBEEF, dtype=np.uint32)
    count = C.c_uint64(7)
    assert lib.fdm_cloud_cluster(0, None, None, None, 0, None, 0, None, 0, None, off_h.ctypes.data_as(C.c_void_p), None,
                                 C.byref(count)) == 0
    assert count.value == 0 and off_h[0] == 0
    # a cloud with an EMPTY list, on the device
    cloud, _ = CC.cases()["spheres"]
    dev = [torch.from_numpy(v).cuda() for v in cloud]
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    off_d = torch.full((1,), 0x5EADBEEF, dtype=torch.int32, device="cuda")
    count = C.c_uint64(7)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    assert lib.fdm_cloud_cluster(100, p(dev[0]), p(dev[1]), p(dev[2]), 1, p(idx), 0, None, 0, None, p(off_d), None,
                                 C.byref(count)) == 0
    assert count.value == 0 and int(off_d.cpu()[0]) == 0
    e = np.zeros(0, dtype=F)
    r = fdm.euclidean_cluster(e, e, e)
    assert r.num_clusters == 0 and r.total_clustered_points == 0 and as_numpy(r.offsets).tolist() == [0]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", sorted(CC.errors()))
def test_undefined_inputs_are_refused(fdm, name, where):
    cloud, kw, word = CC.errors()[name]
    lib = fdm.capi.load()
    n = cloud[0].size
    idx = kw.get("indices")
    m = n if idx is None else idx.size
    cfg = fdm.capi.FdmClusterConfig(float(kw.get("tolerance", 0.5)), 10, 100000)
    count = C.c_uint64(7)
    if where == "host":
        outs = [np.full(m + 1, 0xDEADBEEF, dtype=np.uint32) for _ in range(3)]
        ptrs = [v.ctypes.data_as(C.c_void_p) for v in (*cloud, *outs)]
        p_idx = None if idx is None else idx.ctypes.data_as(C.c_void_p)
    else:
        import torch
        dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in cloud]
        outs = [torch.full((m + 1,), 0x5EADBEEF, dtype=torch.int32, device="cuda") for _ in range(3)]
        ptrs = [C.c_void_p(v.data_ptr()) for v in (*dev, *outs)]
        d_idx = None if idx is None else torch.from_numpy(idx.astype(np.int64)).to(torch.int32).cuda()
        p_idx = None if idx is None else C.c_void_p(d_idx.data_ptr())
        torch.cuda.synchronize()
    rc = lib.fdm_cloud_cluster(n, ptrs[0], ptrs[1], ptrs[2], int(where == "device"), p_idx, m, C.byref(cfg), 0, ptrs[3],
                               ptrs[4], ptrs[5], C.byref(count))
    assert rc == -1, (rc, lib.fdm_last_error())  # FDM_ERR_INVALID
    assert word in lib.fdm_last_error().decode() and count.value == 0
    for v in outs:
        host = v.cpu().numpy() if where == "device" else v
        assert (host == host[0]).all() and int(host[0]) & 0xFFFF == 0xBEEF, "a refused call wrote to an output"
    dev, dev_idx = placed(cloud, where, idx)
    with pytest.raises(fdm.EngineError, match=word):
        fdm.euclidean_cluster(*dev, indices=dev_idx, **{k: v for k, v in kw.items() if k != "indices"})
