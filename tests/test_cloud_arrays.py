"""fastdem_amd/_arrays.py alone, on the CPU: what the adaptor makes of NumPy input, what it refuses without a GPU, the
output conventions; capi.stats_dict; and the names the package exports.
"""
import ctypes as C

import numpy as np
import pytest

import fastdem_amd
from fastdem_amd import capi
from fastdem_amd._arrays import arrays, complement, outputs, to_numpy


def pointed_to(A, a, dtype=np.float32):
    """The values behind ptr(a), read back through the pointer."""
    return np.frombuffer((C.c_char * a.nbytes).from_address(A.ptr(a).value), dtype=dtype).copy()


def test_numpy_inputs_are_converted_in_value():
    wide = np.arange(40, dtype=np.float64).reshape(10, 4) * 0.5
    A = arrays(wide[:, 1], device=3)
    assert (A.on_device, A.device, A.n) == (0, 3, 10)
    for given, got, dtype in ((wide[:, 1], A.f32(wide[:, 1]), np.float32), (wide[::2, 2], A.f32(wide[::2, 2]), np.float32),
                              (np.arange(10, dtype=np.int64)[::-1], A.u32(np.arange(10, dtype=np.int64)[::-1]), np.uint32),
                              ([3, 1, 2], A.index([3, 1, 2]), np.uint32),
                              (np.array([[5, 6], [7, 8]], dtype=np.int16), A.index(np.array([[5, 6], [7, 8]], dtype=np.int16)), np.uint32)):
        assert got.dtype == dtype and got.flags["C_CONTIGUOUS"] and got.ndim == 1
        assert np.array_equal(got, np.asarray(given).reshape(-1))
        assert A.ptr(got).value == got.ctypes.data
    same = np.arange(5, dtype=np.float32)
    assert A.f32(same).ctypes.data == same.ctypes.data                # what the library can read is read in place
    assert A.f32(None) is None and A.u32(None) is None and A.index(None) is None and A.ptr(None) is None
    assert arrays(np.zeros(0, np.float32)).n == 0 and arrays([1.0, 2.0]).n == 2


def test_prepared_arrays_live_as_long_as_the_adaptor():
    A = arrays(np.zeros(3))
    p = A.ptr(A.f32(np.arange(1000, dtype=np.float64)))               # (the only other reference is the adaptor's)
    assert np.array_equal(np.frombuffer((C.c_char * 4000).from_address(p.value), dtype=np.float32), np.arange(1000))


def test_normals_as_one_array_and_as_three():
    rng = np.random.default_rng(1)
    nrm = rng.normal(size=(7, 3))
    A = arrays(nrm[:, 0])
    one, three = A.normals(nrm), A.normals([nrm[:, 0], nrm[:, 1], nrm[:, 2]])
    assert len(one) == len(three) == 3 and A.normals(None) == (None, None, None)
    for k in range(3):
        assert np.array_equal(pointed_to(A, one[k]), nrm[:, k].astype(np.float32))
        assert np.array_equal(pointed_to(A, three[k]), pointed_to(A, one[k]))


def test_covariances_go_column_major():
    cov = np.arange(4 * 9, dtype=np.float64).reshape(4, 3, 3)          # [point][row][column]
    A = arrays(np.zeros(4))
    for given in (cov, cov.reshape(4, 9), cov.astype(np.float32)):
        sent = pointed_to(A, A.cov_colmajor(given, 4)).reshape(4, 3, 3)
        for r in range(3):
            for c in range(3):
                assert np.array_equal(sent[:, c, r], cov[:, r, c])     # value (r, c) at offset 3 c + r
    assert A.cov_colmajor(None, 4) is None


def test_outputs():
    A = arrays(np.zeros(5, np.float32))
    for m in (0, 1, 5):
        buf = A.index_out(m)
        assert buf.dtype == np.uint32 and buf.shape == (max(m, 1),) and not buf.any()
    buf = A.index_out(5)
    buf[:] = [4, 0xFFFFFFFF, 2, 9, 9]
    got = A.take(buf, 3)
    assert got.dtype == np.uint32 and got.tolist() == [4, 0xFFFFFFFF, 2]
    buf[0] = 7
    assert got[0] == 4                                                # a copy
    assert A.zeros((2, 3), "f32").dtype == np.float32 and A.zeros(4, "u8").dtype == np.uint8 and not A.zeros(4, "u8").any()
    assert A.empty((3, 5), "f32").shape == (3, 5) and A.empty(4, "i32").dtype == np.int32
    assert A.empty(6, A.u32(np.arange(6))).dtype == np.uint32         # an output of a prepared input's dtype
    assert A.mask(np.array([1, 0, 1], dtype=np.uint8)).tolist() == [True, False, True]
    H = outputs(None)
    assert (H.on_device, H.device) == (0, 0) and H.zeros(3, "u32").dtype == np.uint32


def test_complement():
    got = complement(np.array([3, 0, 3, 5], dtype=np.uint32), 7)
    assert got.dtype == np.uint32 and got.tolist() == [1, 2, 4, 6]
    assert complement(np.zeros(0, dtype=np.uint32), 3).tolist() == [0, 1, 2] and complement(np.arange(3), 3).size == 0
    assert to_numpy([1, 2]).tolist() == [1, 2]


def test_host_tensors_and_mixed_calls_are_refused():
    torch = pytest.importorskip("torch")
    t = torch.arange(4, dtype=torch.float32)
    with pytest.raises(TypeError):
        arrays(t)                                                     # a CPU tensor as x
    with pytest.raises(TypeError):
        fastdem_amd.cloud.segment_ground(t, t, t)                     # refused before anything touches a device
    A = arrays(np.zeros(4))
    for prepare in (A.f32, A.u32, A.index, lambda v: A.normals(torch.zeros(4, 3)), lambda v: A.normals((v, v, v)),
                    lambda v: A.cov_colmajor(torch.zeros(4, 3, 3), 4)):
        with pytest.raises(TypeError):
            prepare(t)                                                # a tensor anywhere in a NumPy call
    with pytest.raises(TypeError):
        A.xyz(np.zeros(4), t, np.zeros(4))
    assert to_numpy(t).tolist() == [0.0, 1.0, 2.0, 3.0]


def test_stats_dict():
    st = capi.FdmClusterStats(n_points=7, n_components=3, n_kept=2, n_rejected=1, n_clustered=6, candidate_pairs=20, tests=15,
                              neighbour_pairs=9, unions=4, range=1, key_bits=33, ms=(C.c_float * 6)(0.5, 1, 2, 3, 4, 5))
    d = capi.stats_dict(st)
    assert list(d) == [name for name, _ in capi.FdmClusterStats._fields_]
    assert d["n_points"] == 7 and d["key_bits"] == 33 and d["range"] == 1 and d["ms"] == (0.5, 1.0, 2.0, 3.0, 4.0, 5.0)
    assert all(type(v) is int for k, v in d.items() if k != "ms") and all(type(v) is float for v in d["ms"])
    info = capi.FdmVoxelMapInfo(resolution=0.5, inv_resolution=2.0, covariance_epsilon=1e-3, device=1, reserved=9, n_points=10,
                                n_skipped=1, num_voxels=4, n_sparse=2, table_slots=8, max_count=5, max_probe=2,
                                ms=(C.c_float * 3)(1, 2, 3), reserved2=4.0)
    d = capi.stats_dict(info)
    assert set(d) == {"resolution", "inv_resolution", "covariance_epsilon", "device", "n_points", "n_skipped", "num_voxels",
                      "n_sparse", "max_count", "table_slots", "max_probe", "ms"}
    assert not any(k.startswith("reserved") for k in d)
    assert (d["resolution"], d["covariance_epsilon"], d["device"], d["num_voxels"], d["ms"]) == (0.5, 1e-3, 1, 4, (1.0, 2.0, 3.0))
    assert type(d["resolution"]) is float and type(d["covariance_epsilon"]) is float and type(d["table_slots"]) is int


EXPORTED = ["Engine", "EngineError", "HostArray", "host_array", "from_point_cloud", "DEMConfig", "build_dem",
            "statistical_outlier_removal", "sor_last_stats", "voxel_grid", "grid_max_z", "estimate_normals",
            "normals_last_stats", "align_icp", "align_plane_icp", "align_gicp", "linearize", "align_settings",
            "VoxelMap", "align_vgicp", "linearize_vgicp",
            "register_last_stats", "RegistrationResult", "segment_ground", "segment_plane", "segment_multiple_planes",
            "segment_last_stats", "RansacResult", "euclidean_cluster", "apply_cluster_labels",
            "cluster_last_stats", "ClusterResult", "capi", "synth", "pcd"]


def test_the_package_exports_what_it_exported():
    import types
    assert fastdem_amd.__all__ == EXPORTED
    assert all(hasattr(fastdem_amd, name) for name in EXPORTED)
    public = {k for k, v in vars(fastdem_amd).items() if not k.startswith("_") and not isinstance(v, types.ModuleType)}
    assert public == {k for k in EXPORTED if k not in ("capi", "synth", "pcd")}      # (submodules aside) nothing more
