"""Every cloud entry point gives the same bits for NumPy arrays, for contiguous device tensors and for STRIDED device
tensors (columns of one wider tensor), and refuses what fastdem_amd/_arrays.py says it refuses.

The clouds are small cases of the families' own case modules, whose NumPy results the families' tests hold to the
restatements; nothing here is about the algorithms.  One GPU: "the call runs on the tensors' device" is not covered.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

import cluster_cases as CC
import dem_cases as DC
import normal_cases as NC
import reg_cases as RC
import seg_cases as SC
import vgicp_cases as VC

pytestmark = pytest.mark.gpu
F32 = np.float32
FORMS = ("numpy", "contiguous", "strided")


@pytest.fixture(scope="module")
def fdm():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import fastdem_amd
    fastdem_amd.capi.load()
    return fastdem_amd


def strided(a):
    """A device tensor of `a` that is not contiguous: 1-D arrays as a column of an (n, 2) tensor, others with the last
    axis one longer than shown.  uint32 goes as int32, torch's 32-bit integer."""
    import torch
    a = np.asarray(a)
    a = a.view(np.int32) if a.dtype == np.uint32 else a
    if a.ndim == 1:
        return torch.from_numpy(np.stack([a, a[::-1]], axis=1)).cuda()[:, 0]
    wide = np.concatenate([a, a[..., :1]], axis=-1)
    return torch.from_numpy(wide).cuda()[..., :a.shape[-1]]


def forms(**arrays):
    """name -> the keyword arrays in that form; None stays None."""
    on = {k: None if v is None else strided(v) for k, v in arrays.items()}
    assert all(v is None or v.numel() < 2 or not v.is_contiguous() for v in on.values())
    return {"numpy": arrays, "strided": on,
            "contiguous": {k: None if v is None else v.contiguous() for k, v in on.items()}}


def cloud_forms(x, y, z, **channels):
    """The same with x, y, z the columns of ONE (n, 3) tensor p: p[:, 0], p[:, 1], p[:, 2]."""
    import torch
    out = forms(**channels)
    p = torch.from_numpy(np.stack([x, y, z], axis=1)).cuda()
    for name, three in (("numpy", (x, y, z)), ("strided", tuple(p[:, k] for k in range(3))),
                        ("contiguous", tuple(p[:, k].contiguous() for k in range(3)))):
        out[name] = dict(zip("xyz", three), **out[name])
    return out


def xyz(c):
    return c["x"], c["y"], c["z"]


def host(a):
    """A result as NumPy values that compare across the forms: 32-bit integers as the unsigned value (torch's are int32),
    masks as bool."""
    if isinstance(a, (tuple, list)):
        return [host(v) for v in a]
    if isinstance(a, dict):
        return {k: host(v) for k, v in a.items()}
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    if a.dtype in (np.uint32, np.int32, np.int64):
        return (a.view(np.uint32) if a.dtype == np.int32 else a).astype(np.int64)
    return a.astype(bool) if a.dtype in (np.uint8, np.bool_) else a


def assert_same(results, what):
    """results: form -> result (nested tuples / dicts of arrays and scalars); all equal to the NumPy form's, bit for bit."""
    def flat(r):
        r = host(r)
        if isinstance(r, dict):
            return [v for k in sorted(r) for v in flat(r[k])]
        if isinstance(r, list):
            return [v for e in r for v in flat(e)]
        return [r]
    want = flat(results["numpy"])
    for form in FORMS[1:]:
        got = flat(results[form])
        assert len(got) == len(want), (what, form)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, form, i)


def map_bits(eng):
    if eng is None:
        return None
    g = eng.geometry()
    out = {"geometry": np.array([g.length_x, g.length_y, g.resolution, g.position_x, g.position_y, g.rows, g.cols])}
    out.update({name: eng.layer(name).view(np.uint32) for name in eng.layers()})
    eng.close()
    return out


# ---- rasterization, the two filters, buildDEM ----
def test_maps_and_filters(fdm):
    p = DC.pipeline("minus_one_metre")
    cfg = fdm.DEMConfig(**p.config)
    auto, into, floating, sor, dem = {}, {}, {}, {}, {}
    for form, c in cloud_forms(**p.cloud).items():
        p3 = xyz(c)
        auto[form] = map_bits(fdm.from_point_cloud(*p3, cfg.resolution, c["intensity"], c["rgb"], method="mean"))
        eng = fdm.Engine.create_map(8.0, 6.0, cfg.resolution)
        rc, st = eng.from_point_cloud(*p3, c["intensity"], c["rgb"], method="minmax")
        floating[form] = eng.remove_floating_points(*p3, 1.0)
        into[form] = (np.array([rc, st["n_points_used"], st["n_cells_written"]]), map_bits(eng))
        keep, mean, thr = fdm.statistical_outlier_removal(*p3, k=cfg.sor_k, std_mul=cfg.sor_std_mul, return_details=True)
        sor[form] = (keep, mean, np.array(thr))
        eng, st = fdm.build_dem(*p3, c["intensity"], c["rgb"], config=cfg, return_stats=True)
        st.pop("stage_ms")
        dem[form] = ({k: np.array(v) for k, v in st.items()}, map_bits(eng))
    n = p.cloud["x"].size
    assert into["numpy"][0][0] == 0 and 0 < host(sor["numpy"][0]).sum() < n and 0 < host(floating["numpy"]).sum() < n
    assert dem["numpy"][1] is not None and auto["numpy"] is not None
    for results, what in ((auto, "from_point_cloud"), (into, "Engine.from_point_cloud"), (sor, "statistical_outlier_removal"),
                          (floating, "Engine.remove_floating_points"), (dem, "build_dem")):
        assert_same(results, what)


# ---- downsampling and normals ----
def test_downsampling_and_normals(fdm):
    x, y, z = NC.cloud("duplicates")
    n = x.size
    rng = np.random.default_rng(8)
    normals, cov = fdm.estimate_normals(x, y, z, k=10, covariances=True)
    extra = dict(intensity=rng.uniform(0, 1, n).astype(F32), rgb=rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
                 normals=normals, cov=cov.reshape(n, 9))
    voxel, maxz, est = {}, {}, {}
    for form, c in cloud_forms(x, y, z, **extra).items():
        p3 = (c.pop("x"), c.pop("y"), c.pop("z"))
        voxel[form] = fdm.voxel_grid(*p3, 0.25, "nearest", return_index=True, **c)
        maxz[form] = fdm.grid_max_z(*p3, 0.25, return_index=True, **c)
        est[form] = fdm.estimate_normals(*p3, k=10, viewpoint=(0.0, 0.0, 5.0), covariances=True)
    assert 1 < host(voxel["numpy"]["idx"]).size < n and set(voxel["numpy"]) == {"x", "y", "z", "intensity", "rgb", "normals", "cov", "idx"}
    for results, what in ((voxel, "voxel_grid"), (maxz, "grid_max_z"), (est, "estimate_normals")):
        assert_same(results, what)


# ---- registration ----
def registration(res):
    return (res.transform, np.array([res.fitness, res.rmse]), np.array([res.iterations, int(res.converged)]),
            np.zeros(0) if res.covariance is None else res.covariance)


def test_registration(fdm):
    icp = RC.align_case("icp_translation").problem
    T = RC.lin_transforms()[1]
    source, target = cloud_forms(*icp.s), cloud_forms(*icp.t)
    align = {form: registration(fdm.align_icp(*xyz(source[form]), *xyz(target[form]), **dict(icp.set))) for form in FORMS}
    lin = {form: [] for form in FORMS}
    for method in ("plane", "gicp"):
        pr = RC.lin_problem(method, 1, 257, 257)
        source, target, raw = cloud_forms(*pr.s), cloud_forms(*pr.t), forms(**pr.raw)
        for form in FORMS:
            lin[form].append(fdm.linearize(method, *xyz(source[form]), *xyz(target[form]), transform=T,
                                           return_correspondences=True, **raw[form], **dict(pr.set)))
    assert align["numpy"][2][0] > 1 and all(0 < r["num_inliers"] for r in lin["numpy"])
    assert_same(align, "align_icp")
    assert_same(lin, "linearize")


def test_voxelized_gicp(fdm):
    case = VC.align_case("designed_small")
    maps, align = {}, {}
    for form, c in cloud_forms(*case.target).items():
        with fdm.VoxelMap(c["x"], c["y"], c["z"], resolution=case.resolution) as vm:
            info = vm.info()
            info.pop("ms")
            maps[form] = ({k: np.array(v) for k, v in info.items()}, vm.records())
    for form, c in cloud_forms(*case.source, cov=case.source_cov).items():
        with fdm.VoxelMap(*case.target, resolution=case.resolution) as vm:
            align[form] = registration(fdm.align_vgicp(c["x"], c["y"], c["z"], c["cov"], voxel_map=vm, **case.settings))
    assert maps["numpy"][0]["num_voxels"] > 100 and align["numpy"][2][0] > 1
    assert_same(maps, "VoxelMap")
    assert_same(align, "align_vgicp")


# ---- segmentation and clustering ----
def test_segmentation_and_clustering(fdm):
    ground, plane, cluster = {}, {}, {}
    cloud, kw = SC.ground_cases()["n255_edges"]
    for form, c in cloud_forms(*cloud).items():
        ground[form] = fdm.segment_ground(c["x"], c["y"], c["z"], **kw)
    cloud, kw = SC.plane_cases()["scene45_third"]
    kw = dict(kw)
    for form, c in cloud_forms(*cloud, indices=kw.pop("indices")).items():
        r = fdm.segment_plane(c["x"], c["y"], c["z"], indices=c["indices"], **kw)
        plane[form] = (r.coefficients, r.inliers, np.array([r.fitness, r.iterations, r.success]), r.outliers(cloud[0].size))
    cloud, kw = CC.cases()["ground_subset"]
    kw = dict(kw)
    for form, c in cloud_forms(*cloud, indices=kw.pop("indices")).items():
        r = fdm.euclidean_cluster(c["x"], c["y"], c["z"], indices=c["indices"], **kw)
        cluster[form] = (r.indices, r.offsets, r.labels, r.noise_indices(cloud[0].size), fdm.apply_cluster_labels(r, cloud[0].size))
    assert sum(host(v).size for v in ground["numpy"]) == 255 and plane["numpy"][2][2] and host(cluster["numpy"][1]).size > 1
    for results, what in ((ground, "segment_ground"), (plane, "segment_plane"), (cluster, "euclidean_cluster")):
        assert_same(results, what)


# ---- PCD ----
def test_pcd_encode(fdm):
    p = DC.pipeline("minus_one_metre").cloud
    nx, ny, nz = NC.surface(p["x"].size, 9)
    out = {form: np.frombuffer(fdm.pcd.encode(c), dtype=np.uint8) for form, c in cloud_forms(**p, nx=nx, ny=ny, nz=nz).items()}
    assert out["numpy"].size == p["x"].size * 32
    assert_same(out, "pcd.encode")


# ---- what is refused, what is still taken ----
def test_refusals(fdm):
    import torch
    cloud, kw = SC.plane_cases()["scene45_third"]
    dev = [torch.from_numpy(np.array(v)).cuda() for v in cloud]
    with pytest.raises(TypeError):
        fdm.segment_ground(*[v.double() for v in dev])
    with pytest.raises(TypeError):
        fdm.from_point_cloud(*[v.double() for v in dev], 0.5)
    with pytest.raises(TypeError):                                   # a NumPy index list in a tensor call
        fdm.segment_plane(*dev, distance_threshold=0.05, indices=kw["indices"])
    with pytest.raises(TypeError):                                   # and a tensor in a NumPy call
        fdm.segment_plane(*cloud, distance_threshold=0.05, indices=torch.from_numpy(kw["indices"].astype(np.int64)).cuda())
    with pytest.raises(TypeError):                                   # a host tensor is no device tensor
        fdm.segment_ground(*[v.cpu() for v in dev])
    with pytest.raises(TypeError):
        fdm.build_dem(dev[0], dev[1], dev[2], rgb=torch.zeros(dev[0].numel(), dtype=torch.int64, device="cuda"))


def test_float64_numpy_arrays_are_taken_everywhere(fdm):
    p = DC.pipeline("minus_one_metre")
    x, y, z = (p.cloud[k] for k in "xyz")
    d = [v.astype(np.float64) for v in (x, y, z)]
    wide = np.stack(d, axis=1)                                       # its columns: float64 and strided
    idx = np.arange(0, x.size, 3)
    cfg = fdm.DEMConfig(**p.config)
    nrm, cov = fdm.estimate_normals(x, y, z, k=10, covariances=True)
    nrm64, cov64 = nrm.astype(np.float64), cov.astype(np.float64)
    eng = fdm.Engine.create_map(8.0, 6.0, 0.2)

    def raster(a):
        e = fdm.Engine.create_map(8.0, 6.0, 0.2)
        return np.array(e.from_point_cloud(*a)[0]), map_bits(e)

    def voxel_map(a):
        with fdm.VoxelMap(*a, resolution=0.5) as vm:
            return vm.records()

    def vgicp(a, c):
        return registration(fdm.align_vgicp(*a, c, target=(x, y, z), voxel_resolution=0.5, max_iterations=3))

    def plane(a):
        r = fdm.segment_plane(*a, distance_threshold=0.05, indices=idx)
        return r.coefficients, r.inliers

    def cluster(a):
        r = fdm.euclidean_cluster(*a, indices=idx, tolerance=0.3)
        return r.indices, r.offsets, r.labels

    calls = {
        "from_point_cloud": lambda a: map_bits(fdm.from_point_cloud(*a, 0.2)),
        "Engine.from_point_cloud": raster,
        "Engine.remove_floating_points": lambda a: eng.remove_floating_points(*a, 1.0),
        "statistical_outlier_removal": lambda a: fdm.statistical_outlier_removal(*a, k=8),
        "build_dem": lambda a: map_bits(fdm.build_dem(*a, config=cfg)),
        "voxel_grid": lambda a: fdm.voxel_grid(*a, 0.25, return_index=True),
        "grid_max_z": lambda a: fdm.grid_max_z(*a, 0.25, return_index=True),
        "estimate_normals": lambda a: fdm.estimate_normals(*a, k=10),
        "align_icp": lambda a: registration(fdm.align_icp(*a, x, y, z, max_iterations=3)),
        "linearize": lambda a: fdm.linearize("icp", *a, x, y, z),
        "VoxelMap": voxel_map,
        "segment_ground": lambda a: fdm.segment_ground(*a),
        "segment_plane": plane,
        "euclidean_cluster": cluster,
        "pcd.encode": lambda a: np.frombuffer(fdm.pcd.encode(dict(zip("xyz", a))), dtype=np.uint8),
    }
    for what, call in calls.items():
        assert_same({"numpy": call((x, y, z)), "contiguous": call(d), "strided": call([wide[:, k] for k in range(3)])}, what)
    # the channels that are not coordinates
    assert_same({"numpy": fdm.linearize("plane", x, y, z, x, y, z, target_normals=nrm),
                 "contiguous": fdm.linearize("plane", *d, *d, target_normals=nrm64),
                 "strided": fdm.linearize("plane", *d, *d, target_normals=tuple(nrm64[:, k] for k in range(3)))}, "normals")
    assert_same({"numpy": vgicp((x, y, z), cov), "contiguous": vgicp(d, cov64), "strided": vgicp(d, cov64.reshape(-1, 9))},
                "covariances")
    eng.close()
