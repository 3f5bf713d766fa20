"""The cloud library over the C ABI (include/fdm_engine.h): rasterization, outlier removal (statistical and radius), the
crop filters, buildDEM, downsampling, normals, registration (ICP, plane ICP, GICP, VGICP), segmentation and clustering.

Every function takes NumPy arrays (staged by the library) or torch device tensors (read in place); _arrays.py states
what that means, once, for all of them.
"""
import ctypes as C

import numpy as np

from . import capi
from ._arrays import arrays, complement, to_numpy
from .capi import FdmCloudOut, FdmCloudView, FdmDemConfig, FdmDemStats, FdmRasterStats, stats_dict
from .engine import Engine, EngineError, _ck, _colmajor16, _ptr, _raster_method


def from_point_cloud(x, y, z, resolution, intensity=None, rgb=None, method="max", device=0):
    """fastdem::fromPointCloud(cloud, resolution, method): a map-only Engine sized to the cloud's x / y bounding box
    (found on the device) with the cloud rasterized into it; None for an empty cloud.  numpy arrays or torch device
    tensors.  A cloud without a finite, positive extent (every x or y NaN, an infinite coordinate) raises EngineError."""
    A = arrays(x, device)
    h, st = C.c_void_p(), FdmRasterStats()
    rc = _ck(capi.load().fdm_engine_create_from_point_cloud(
        A.n, *A.cloud5(x, y, z, intensity, rgb), A.on_device, float(np.float32(resolution)), _raster_method(method),
        A.device, C.byref(h), C.byref(st)))
    if rc != 0 or not h.value:
        return None
    return Engine._adopt(h)


class DEMConfig:
    """fastdem::DEMConfig (io/pcd_convert.hpp:28-42), with the reference's defaults."""

    def __init__(self, resolution=0.1, method="max", sor_k=10, sor_std_mul=1.0, height_threshold=2.0, bin_size=0.0,
                 inpaint_iterations=3):
        self.resolution, self.method = resolution, method
        self.sor_k, self.sor_std_mul = sor_k, sor_std_mul
        self.height_threshold, self.bin_size = height_threshold, bin_size
        self.inpaint_iterations = inpaint_iterations

    def as_struct(self):
        return FdmDemConfig(float(np.float32(self.resolution)), _raster_method(self.method), int(self.sor_k),
                            float(np.float32(self.sor_std_mul)), float(np.float32(self.height_threshold)),
                            float(np.float32(self.bin_size)), int(self.inpaint_iterations))


def _last_stats(struct, getter):
    st = struct()
    _ck(getattr(capi.load(), getter)(C.byref(st)))
    return stats_dict(st)


def sor_last_stats():
    """What this thread's last outlier removal did: n_queries, n_fallback (queries the brute-force queue took), grid_x,
    grid_y, voxel, ms (grid build, search, fallback queue, statistics)."""
    return _last_stats(capi.FdmSorStats, "fdm_sor_last_stats")


def statistical_outlier_removal(x, y, z, k=10, std_mul=1.0, device=0, return_details=False):
    """nanopcl::filters::statisticalOutlierRemoval(cloud, k, std_mul) as a keep mask over the input points: bool[n] for
    numpy arrays, a torch uint8 device tensor for torch device tensors.  return_details: (keep, mean_dist, threshold)
    with mean_dist the per-point mean distance to its k nearest neighbours (float32) and threshold a np.float32."""
    A = arrays(x, device)
    p = A.xyz(x, y, z)
    thr, n_kept = C.c_float(0.0), C.c_uint64(0)
    keep8, mean = A.zeros(A.n, "u8"), A.zeros(A.n, "f32")
    _ck(capi.load().fdm_statistical_outlier_removal(A.n, *p, A.on_device, int(k), float(np.float32(std_mul)), A.device,
                                                    A.ptr(keep8), A.ptr(mean), C.byref(thr), C.byref(n_kept)))
    assert int(keep8.sum()) == n_kept.value
    keep = A.mask(keep8)
    return (keep, mean, np.float32(thr.value)) if return_details else keep


# ---- radius outlier removal, the crop family, removeInvalid (fdm_cloud_radius_outlier_removal / fdm_cloud_crop) ----
def radius_outlier_removal(x, y, z, radius, min_neighbors, device=0, return_counts=False):
    """nanopcl::filters::radiusOutlierRemoval(cloud, radius, min_neighbors) as a keep mask over the input points: bool[n]
    for numpy arrays, a torch uint8 device tensor for torch device tensors.  A point stays iff at least min_neighbors
    OTHER points (by index: a duplicate counts) lie within `radius` of it; the relation is stated in include/fdm_engine.h.
    return_counts: (keep, counts) with the exact neighbour count of every point (uint32, int32 for tensors) — the whole
    neighbourhood is then walked; without it a point's search stops at min_neighbors.  A coordinate that is not finite is
    refused: remove_invalid first."""
    A = arrays(x, device)
    p = A.xyz(x, y, z)
    n_kept = C.c_uint64(0)
    keep8 = A.zeros(A.n, "u8")
    counts = A.zeros(A.n, "u32") if return_counts else None
    _ck(capi.load().fdm_cloud_radius_outlier_removal(A.n, *p, A.on_device, float(np.float32(radius)), int(min_neighbors),
                                                     A.device, A.ptr(keep8), A.ptr(counts), C.byref(n_kept)))
    assert int(keep8.sum()) == n_kept.value
    keep = A.mask(keep8)
    return (keep, counts) if return_counts else keep


def ror_last_stats():
    """What this thread's last radius_outlier_removal did: n_points, candidate_tests (the work bound's measure),
    tests_done, n_kept, range, key_bits, ms (voxels, sort, candidate tests, the count kernel, the outputs' way back; zeros
    unless fdm_cloud_debug_profile is on)."""
    return _last_stats(capi.FdmRorStats, "fdm_ror_last_stats")


def _crop(kind, x, y, z, lo, hi, mode, device):
    A = arrays(x, device)
    p = A.xyz(x, y, z)
    f3 = lambda v: (C.c_float * 3)(*[float(np.float32(c)) for c in v])  # noqa: E731
    cfg = capi.FdmCropConfig(capi.CROP_KIND[kind], capi.CROP_MODE[mode.lower()] if isinstance(mode, str) else int(mode),
                             f3(lo), f3(hi))
    n_kept = C.c_uint64(0)
    keep8 = A.zeros(A.n, "u8")
    _ck(capi.load().fdm_cloud_crop(A.n, *p, A.on_device, C.byref(cfg), A.device, A.ptr(keep8), C.byref(n_kept)))
    assert int(keep8.sum()) == n_kept.value
    return A.mask(keep8)


def crop_box(x, y, z, lo, hi, mode="inside", device=0):
    """nanopcl::filters::cropBox(cloud, min, max, mode) as a keep mask (as radius_outlier_removal returns it): "inside"
    keeps lo <= p <= hi on every axis, "outside" what lies below lo or above hi on some axis.  Like every crop here the
    predicate is the reference's, comparison by comparison: a NaN coordinate fails each comparison it is in."""
    return _crop("box", x, y, z, lo, hi, mode, device)


def crop_range(x, y, z, min_range, max_range, mode="inside", device=0):
    """cropRange: the squared distance from the origin against min_range^2 and max_range^2 (fp32).  A keep mask."""
    return _crop("range", x, y, z, (min_range, 0, 0), (max_range, 0, 0), mode, device)


def crop_x(x, y, z, lo, hi, mode="inside", device=0):
    """cropX: lo <= x <= hi ("outside": x < lo or x > hi).  A keep mask."""
    return _crop("x", x, y, z, (lo, 0, 0), (hi, 0, 0), mode, device)


def crop_y(x, y, z, lo, hi, mode="inside", device=0):
    """cropY, as crop_x."""
    return _crop("y", x, y, z, (lo, 0, 0), (hi, 0, 0), mode, device)


def crop_z(x, y, z, lo, hi, mode="inside", device=0):
    """cropZ, as crop_x."""
    return _crop("z", x, y, z, (lo, 0, 0), (hi, 0, 0), mode, device)


def crop_angle(x, y, z, min_angle, max_angle, mode="inside", device=0):
    """cropAngle: the azimuth sector from min_angle to max_angle (radians, counter-clockwise; min > max wraps through pi),
    by the reference's cross products against eps = 1e-5.  A keep mask."""
    return _crop("angle", x, y, z, (min_angle, 0, 0), (max_angle, 0, 0), mode, device)


def remove_invalid(x, y, z, device=0):
    """nanopcl::filters::removeInvalid as a keep mask: the points whose three coordinates are finite."""
    return _crop("finite", x, y, z, (0, 0, 0), (0, 0, 0), "inside", device)


def build_dem(x, y, z, intensity=None, rgb=None, config=None, device=0, return_stats=False):
    """fastdem::buildDEM(cloud, config): outlier removal, floating-point removal, rasterization and inpainting on the
    device.  Returns a map-only Engine, or None where the reference returns an uninitialised map (an empty cloud, a
    cloud the outlier removal empties).  numpy arrays or torch device tensors.  return_stats: (engine, dict of
    fdm_dem_stats)."""
    A = arrays(x, device)
    cfg = (config if config is not None else DEMConfig()).as_struct()
    h, st = C.c_void_p(), FdmDemStats()
    rc = _ck(capi.load().fdm_engine_build_dem(A.n, *A.cloud5(x, y, z, intensity, rgb), A.on_device, C.byref(cfg),
                                              A.device, C.byref(h), C.byref(st)))
    eng = Engine._adopt(h) if rc == 0 and h.value else None
    if not return_stats:
        return eng
    stats = {"status": rc, "n_input": int(st.n_input), "n_after_sor": int(st.n_after_sor),
             "n_after_height": int(st.n_after_height), "n_sor_fallback": int(st.n_sor_fallback),
             "sor_threshold": np.float32(st.sor_threshold), "stage_ms": tuple(float(v) for v in st.stage_ms),
             "n_points_used": int(st.raster.n_points_used), "n_cells_written": int(st.raster.n_cells_written)}
    return eng, stats


def _downsample(x, y, z, size, mode, intensity, rgb, normals, cov, order, device, return_index):
    """fdm_cloud_voxel_grid (mode 0 .. 3) / fdm_cloud_grid_max_z (mode None) on numpy arrays or torch device tensors."""
    lib = capi.load()
    A = arrays(x, device)
    n = A.n
    given = {"x": A.f32(x), "y": A.f32(y), "z": A.f32(z), "intensity": A.f32(intensity), "rgb": A.u32(rgb),
             "cov9": A.f32(cov)}
    given.update(zip(("nx", "ny", "nz"), A.normals(normals)))
    outs = {k: A.empty((n, 9) if k == "cov9" else n, v) for k, v in given.items() if v is not None}
    outs["idx"] = A.empty(n, "u32")
    view = FdmCloudView(**{k: A.ptr(v) for k, v in given.items()})
    out = FdmCloudOut(**{k: A.ptr(v) for k, v in outs.items()})
    n_out = C.c_uint64(0)
    size = float(np.float32(size))
    if mode is None:
        _ck(lib.fdm_cloud_grid_max_z(n, C.byref(view), A.on_device, size, int(order), A.device, C.byref(out),
                                     C.byref(n_out)))
    else:
        m = capi.VOXEL_MODE[mode.lower()] if isinstance(mode, str) else int(mode)
        _ck(lib.fdm_cloud_voxel_grid(n, C.byref(view), A.on_device, size, m, int(order), A.device, C.byref(out),
                                     C.byref(n_out)))
    k = int(n_out.value)
    idx = outs.pop("idx")
    res = {name: v[:k] for name, v in outs.items()}
    if "nx" in res:
        res["normals"] = (res.pop("nx"), res.pop("ny"), res.pop("nz"))
    if "cov9" in res:
        res["cov"] = res.pop("cov9")
    if return_index:
        res["idx"] = A.take(idx, k)
    return res


def voxel_grid(x, y, z, voxel_size, mode="centroid", intensity=None, rgb=None, normals=None, cov=None, order=0,
               device=0, return_index=False):
    """nanopcl::filters::voxelGrid(cloud, voxel_size, mode) on the device: mode "centroid", "nearest", "any" or "center".
    numpy arrays in, numpy arrays out; torch device tensors in, device tensors out (they can feed integrate_device or
    from_point_cloud as they are).  normals: three arrays (nx, ny, nz) or one of shape (n, 3); cov: (n, 9).  Returns a
    dict with "x", "y", "z" and the channels given ("intensity", "rgb", "normals" as a tuple of three, "cov");
    return_index adds "idx", the input index each output point was copied from (centroid, center: the voxel's
    representative).  order: 0 = ties in input order, 1 = the order std::sort leaves (engine option "voxel_any_order").
    device: the ordinal numpy input runs on; torch tensors run on the device they live on."""
    return _downsample(x, y, z, voxel_size, mode, intensity, rgb, normals, cov, order, device, return_index)


def grid_max_z(x, y, z, grid_size, intensity=None, rgb=None, normals=None, cov=None, order=0, device=0,
               return_index=False):
    """nanopcl::filters::gridMaxZ(cloud, grid_size) on the device: per (x, y) cell the point with the largest z, every
    channel that point's.  Arguments and result as voxel_grid."""
    return _downsample(x, y, z, grid_size, None, intensity, rgb, normals, cov, order, device, return_index)


def normals_last_stats():
    """What this thread's last estimate_normals did: n_queries, n_fallback (queries the brute-force queue took),
    n_invalid, grid_x, grid_y, voxel, ms (grid build, search, fallback queue, write; zeros unless
    fdm_cloud_debug_profile is on)."""
    return _last_stats(capi.FdmNormalStats, "fdm_normals_last_stats")


def estimate_normals(x, y, z, k=20, viewpoint=(0.0, 0.0, 0.0), covariances=False, device=0, return_stats=False):
    """nanopcl::geometry::estimateNormals(cloud, k, viewpoint) on the device, or estimateNormalsCovariances with
    covariances=True: per point the PCA of its k nearest points (itself included), the normal turned towards the
    viewpoint, the covariance regularised for GICP to eigenvalues (1e-3, 1, 1).  numpy arrays in, numpy arrays out; torch
    device tensors in, device tensors out.  Returns normals[n, 3], or (normals, cov[n, 3, 3]) with covariances; points
    with fewer than 3 neighbours or a degenerate neighbourhood get a zero normal and the identity.  return_stats appends
    normals_last_stats().  device: the ordinal numpy input runs on; torch tensors run on the device they live on."""
    A = arrays(x, device)
    n = A.n
    vp = (C.c_float * 3)(*[float(np.float32(v)) for v in viewpoint])
    n_invalid = C.c_uint64(0)
    soa = A.empty((3, n), "f32")
    cov9 = A.empty((n, 9), "f32") if covariances else None
    _ck(capi.load().fdm_cloud_estimate_normals(n, *A.xyz(x, y, z), A.on_device, int(k), vp, A.device, A.ptr(soa[0]),
                                               A.ptr(soa[1]), A.ptr(soa[2]), A.ptr(cov9), C.byref(n_invalid)))
    out = (A.compact(soa.T),)
    if covariances:
        out += (A.compact(cov9.reshape(n, 3, 3).swapaxes(1, 2)),)    # column-major -> [row][column]
    if return_stats:
        out += (normals_last_stats(),)
    return out[0] if len(out) == 1 else out


class RegistrationResult:
    """nanopcl::registration::RegistrationResult: transform (4 x 4, source -> target), fitness, rmse, iterations,
    converged and covariance (6 x 6 in [v; omega] order, or None)."""

    __slots__ = ("transform", "fitness", "rmse", "iterations", "converged", "covariance")

    def __init__(self, transform, fitness, rmse, iterations, converged, covariance):
        self.transform, self.fitness, self.rmse = transform, fitness, rmse
        self.iterations, self.converged, self.covariance = iterations, converged, covariance

    def success(self, min_fitness=0.5):
        return self.converged and self.fitness >= min_fitness

    def information_matrix(self):
        return None if self.covariance is None else np.linalg.inv(self.covariance)

    def __repr__(self):
        return (f"RegistrationResult(fitness={self.fitness:.4g}, rmse={self.rmse:.4g}, iterations={self.iterations}, "
                f"converged={self.converged}, covariance={'yes' if self.covariance is not None else 'None'})")


def align_settings(**settings):
    """fdm_align_settings with AlignSettings' defaults and the given fields: max_correspondence_dist, max_iterations,
    translation_eps, rotation_eps, relative_error_eps, min_correspondences, robust_kernel ("none", "huber", "tukey",
    "cauchy" or its number), robust_kernel_width, covariance_epsilon."""
    st = capi.FdmAlignSettings()
    capi.load().fdm_default_align_settings(C.byref(st))
    names = {f[0] for f in capi.FdmAlignSettings._fields_} - {"reserved"}
    for key, value in settings.items():
        if key not in names:
            raise TypeError(f"unknown registration setting {key!r}")
        if key == "robust_kernel" and isinstance(value, str):
            value = capi.ROBUST_KERNEL[value.lower()]
        setattr(st, key, value)
    return st


def _registration_result(res):
    """RegistrationResult of an FdmRegistrationResult."""
    T = np.array(res.transform, dtype=np.float64).reshape(4, 4).T.copy()
    cov = np.array(res.covariance, dtype=np.float64).reshape(6, 6) if res.has_covariance else None
    return RegistrationResult(T, float(res.fitness), float(res.rmse), int(res.iterations), bool(res.converged), cov)


def _linearized(entry, A, n, return_correspondences):
    """The outputs of one linearize entry: makes H, b, error, num_inliers and (asked for) corr — n int32 where the clouds
    of adaptor A live —, calls entry(H, b, error, num_inliers, corr) and returns the result dict."""
    H, b = (C.c_double * 21)(), (C.c_double * 6)()
    err, cnt = C.c_double(0.0), C.c_uint64(0)
    corr = A.empty(n, "i32") if return_correspondences else None
    _ck(entry(H, b, C.byref(err), C.byref(cnt), A.ptr(corr)))
    Hu = np.array(H, dtype=np.float64)
    full = np.zeros((6, 6))
    full[np.triu_indices(6)] = Hu
    full = full + np.triu(full, 1).T
    out = {"H": full, "H_upper": Hu, "b": np.array(b, dtype=np.float64), "error": float(err.value),
           "num_inliers": int(cnt.value)}
    if return_correspondences:
        out["corr"] = corr
    return out


def _register_clouds(A, source, target, target_normals, source_cov, target_cov):
    """The FdmRegisterClouds of a call; adaptor A (of the source's x) holds the arrays it points into."""
    tx, ty, tz = (A.f32(v) for v in target)
    ns, nt = A.n, len(tx)
    return capi.FdmRegisterClouds(ns, *A.xyz(*source), A.ptr(A.cov_colmajor(source_cov, ns)), nt, A.ptr(tx), A.ptr(ty),
                                  A.ptr(tz), *[A.ptr(v) for v in A.normals(target_normals)],
                                  A.ptr(A.cov_colmajor(target_cov, nt)), A.on_device)


def _guess16(T):
    return None if T is None else (C.c_double * 16)(*_colmajor16(T))


def _register(method, source, target, initial_guess, target_normals, source_cov, target_cov, device, settings):
    A = arrays(source[0], device)
    clouds = _register_clouds(A, source, target, target_normals, source_cov, target_cov)
    st = settings.pop("settings", None) or align_settings(**settings)
    res = capi.FdmRegistrationResult()
    _ck(capi.load().fdm_cloud_register(capi.REGISTER_METHOD[method], C.byref(clouds), _guess16(initial_guess),
                                       C.byref(st), A.device, C.byref(res)))
    return _registration_result(res)


def align_icp(sx, sy, sz, tx, ty, tz, initial_guess=None, device=0, **settings):
    """nanopcl::registration::alignICP(source, target, initial_guess, settings) on the device: point-to-point ICP.
    numpy arrays or torch device tensors (they run on the device they live on); initial_guess a 4 x 4 matrix (None = the
    identity); settings: the fields of AlignSettings by name (align_settings).  Returns a RegistrationResult."""
    return _register("icp", (sx, sy, sz), (tx, ty, tz), initial_guess, None, None, None, device, settings)


def align_plane_icp(sx, sy, sz, tx, ty, tz, target_normals, initial_guess=None, device=0, **settings):
    """alignPlaneICP: point-to-plane ICP against the target's normals (three arrays or one of shape (n, 3), e.g. from
    estimate_normals).  Otherwise as align_icp."""
    return _register("plane", (sx, sy, sz), (tx, ty, tz), initial_guess, target_normals, None, None, device, settings)


def align_gicp(sx, sy, sz, tx, ty, tz, source_cov, target_cov, initial_guess=None, device=0, **settings):
    """alignGICP: generalized ICP with both clouds' covariances, (n, 3, 3) indexed [row][column] as
    estimate_normals(..., covariances=True) returns them.  Otherwise as align_icp."""
    return _register("gicp", (sx, sy, sz), (tx, ty, tz), initial_guess, None, source_cov, target_cov, device, settings)


def linearize(method, sx, sy, sz, tx, ty, tz, transform=None, target_normals=None, source_cov=None, target_cov=None,
              device=0, return_correspondences=False, **settings):
    """One linearization of `method` ("icp", "plane", "gicp") at `transform` — the reference's linearizer: a dict with H
    (6 x 6, symmetric), H_upper (21), b (6), error and num_inliers; return_correspondences adds "corr", the target index
    of every source point (-1 for none)."""
    A = arrays(sx, device)
    clouds = _register_clouds(A, (sx, sy, sz), (tx, ty, tz), target_normals, source_cov, target_cov)
    st = settings.pop("settings", None) or align_settings(**settings)
    lib, number = capi.load(), capi.REGISTER_METHOD[method]
    return _linearized(lambda *out: lib.fdm_cloud_register_linearize(number, C.byref(clouds), _guess16(transform),
                                                                     C.byref(st), A.device, *out),
                       A, A.n, return_correspondences)


def register_last_stats():
    """What this thread's last registration call did: n_source, n_target, grid_x, grid_y, voxel (the target's search
    grid), ring_limit, linearizations, ms (grid build, regularisation, the linearizations summed; zeros unless
    fdm_cloud_debug_profile is on)."""
    return _last_stats(capi.FdmRegisterStats, "fdm_register_last_stats")


# ---- voxelized GICP (fdm_voxel_map_* / fdm_cloud_register_vgicp: include/fdm_engine.h) ----
class VoxelMap:
    """nanopcl::registration::VoxelDistributionMap on the device: per-voxel means and covariances of a target cloud, built
    once and registered against any number of times (align_vgicp, linearize_vgicp).  x, y, z: NumPy arrays, or torch
    device tensors (the map then lives on their device).  Owns device memory until close() (or the end of a `with`)."""

    def __init__(self, x, y, z, resolution=1.0, covariance_epsilon=1e-3, device=0):
        self._h = None
        A = arrays(x, device)
        h = C.c_void_p()
        _ck(capi.load().fdm_voxel_map_create(A.n, *A.xyz(x, y, z), A.on_device, float(resolution),
                                             float(covariance_epsilon), A.device, C.byref(h)))
        self._h = h

    def close(self):
        h, self._h = self._h, None
        if h:
            capi.load().fdm_voxel_map_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _handle(self):
        if not self._h:
            raise EngineError("the voxel map is closed")
        return self._h

    def info(self):
        """dict: resolution, inv_resolution, covariance_epsilon, device, n_points, n_skipped (not finite), num_voxels,
        n_sparse (fewer than 3 points), max_count, table_slots, max_probe, ms (keys + sort, reduce + regularise, hash:
        zeros unless fdm_cloud_debug_profile was on)."""
        st = capi.FdmVoxelMapInfo()
        _ck(capi.load().fdm_voxel_map_get_info(self._handle(), C.byref(st)))
        return stats_dict(st)

    def __len__(self):
        return int(self.info()["num_voxels"])

    def records(self):
        """dict of NumPy arrays in ascending key order: key uint64[m], count uint32[m], mean float32[m, 3], cov
        float32[m, 3, 3] and creg float64[m, 3, 3] (the regularised covariance), both indexed [row][column]."""
        m = len(self)
        key, count = np.empty(m, dtype=np.uint64), np.empty(m, dtype=np.uint32)
        mean, cov9 = np.empty((m, 3), dtype=np.float32), np.empty((m, 9), dtype=np.float32)
        c6 = np.empty((m, 6), dtype=np.float64)
        _ck(capi.load().fdm_voxel_map_records(self._handle(), 0, _ptr(key), _ptr(mean), _ptr(cov9), _ptr(c6), _ptr(count)))
        creg = c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(m, 3, 3)
        return {"key": key, "count": count, "mean": mean,
                "cov": np.ascontiguousarray(cov9.reshape(m, 3, 3).transpose(0, 2, 1)), "creg": np.ascontiguousarray(creg)}


def _vgicp_map(voxel_map, target, voxel_resolution, st, device):
    """(the map to use, whether it is this call's to close)."""
    if (voxel_map is None) == (target is None):
        raise TypeError("give exactly one of voxel_map and target")
    if voxel_map is not None:
        return voxel_map, False
    tx, ty, tz = target
    return VoxelMap(tx, ty, tz, voxel_resolution, st.covariance_epsilon, device), True


def align_vgicp(sx, sy, sz, source_cov, voxel_map=None, target=None, voxel_resolution=1.0, initial_guess=None, device=0,
                **settings):
    """nanopcl::registration::alignVGICP on the device.  Give a prebuilt VoxelMap (the fast path: one lookup per point
    and iteration), or target=(tx, ty, tz), which builds a map of voxel_resolution with settings' covariance_epsilon for
    this call alone.  source_cov: (n, 3, 3) indexed [row][column].  max_correspondence_dist is not used.  Otherwise as
    align_icp."""
    st = settings.pop("settings", None) or align_settings(**settings)
    vmap, mine = _vgicp_map(voxel_map, target, voxel_resolution, st, device)
    try:
        A = arrays(sx, device)
        res = capi.FdmRegistrationResult()
        _ck(capi.load().fdm_cloud_register_vgicp(vmap._handle(), A.n, *A.xyz(sx, sy, sz),
                                                 A.ptr(A.cov_colmajor(source_cov, A.n)), A.on_device,
                                                 _guess16(initial_guess), C.byref(st), C.byref(res)))
    finally:
        if mine:
            vmap.close()
    return _registration_result(res)


def linearize_vgicp(sx, sy, sz, source_cov, voxel_map=None, target=None, voxel_resolution=1.0, transform=None, device=0,
                    return_correspondences=False, **settings):
    """One VGICP linearization at `transform`, shaped like linearize: H, H_upper, b, error, num_inliers, and with
    return_correspondences "corr": every source point's voxel as its rank in ascending key order (-1 for none)."""
    st = settings.pop("settings", None) or align_settings(**settings)
    vmap, mine = _vgicp_map(voxel_map, target, voxel_resolution, st, device)
    try:
        A = arrays(sx, device)
        source = (A.n, *A.xyz(sx, sy, sz), A.ptr(A.cov_colmajor(source_cov, A.n)), A.on_device)
        lib = capi.load()
        return _linearized(lambda *out: lib.fdm_cloud_register_vgicp_linearize(vmap._handle(), *source,
                                                                               _guess16(transform), C.byref(st), *out),
                           A, A.n, return_correspondences)
    finally:
        if mine:
            vmap.close()


# ---- cloud segmentation (fdm_cloud_segment_ground / _plane / _planes: include/fdm_engine.h) ----
def segment_ground(x, y, z, grid_resolution=0.5, cell_percentile=0.2, ground_thickness=0.3, max_ground_height=0.5,
                   min_points_per_cell=2, device=0):
    """nanopcl::segmentation::segmentGround(cloud, config) on the device: (ground, obstacles), the point indices of each
    in ascending order — uint32 numpy arrays for numpy input, int64 device tensors for torch device tensors."""
    A = arrays(x, device)
    p = A.xyz(x, y, z)
    cfg = capi.FdmGroundSegConfig(float(np.float32(grid_resolution)), float(np.float32(cell_percentile)),
                                  float(np.float32(ground_thickness)), float(np.float32(max_ground_height)),
                                  int(min_points_per_cell))
    ground, obstacles = A.index_out(A.n), A.index_out(A.n)
    ng, no = C.c_uint64(0), C.c_uint64(0)
    _ck(capi.load().fdm_cloud_segment_ground(A.n, *p, A.on_device, C.byref(cfg), A.device, A.ptr(ground),
                                             A.ptr(obstacles), C.byref(ng), C.byref(no)))
    return A.take(ground, int(ng.value)), A.take(obstacles, int(no.value))


class RansacResult:
    """nanopcl::segmentation::RansacResult: coefficients (float32[4]: nx, ny, nz, d), inliers (indices into the cloud, in
    index-list order), fitness, iterations, success."""

    def __init__(self, coefficients, inliers, fitness, iterations, success):
        self.coefficients, self.inliers = coefficients, inliers
        self.fitness, self.iterations, self.success = float(fitness), int(iterations), bool(success)

    def outliers(self, total):
        """RansacResult::outliers(total_points): the indices 0 .. total - 1 that are no inlier, ascending."""
        return complement(self.inliers, total)

    def __repr__(self):
        return (f"RansacResult(success={self.success}, coefficients={self.coefficients.tolist()}, "
                f"inliers={len(self.inliers)}, fitness={self.fitness:.6f}, iterations={self.iterations})")


def _ransac_config(distance_threshold, max_iterations, probability, min_inliers, refine_model):
    return capi.FdmRansacConfig(float(np.float32(distance_threshold)), int(max_iterations), float(probability),
                                int(min_inliers), 1 if refine_model else 0)


def _ransac_result(A, r, inliers):
    return RansacResult(np.array(r.coefficients, dtype=np.float32), A.take(inliers, int(r.n_inliers)),
                        r.fitness, r.iterations, r.success)


def segment_plane(x, y, z, distance_threshold=0.1, max_iterations=1000, probability=0.99, min_inliers=3,
                  refine_model=True, indices=None, device=0):
    """nanopcl::segmentation::segmentPlane (RANSAC, fixed seed) over the whole cloud or over `indices` (positions are
    sampled in that list, which may repeat a point).  Returns a RansacResult; its inliers are a uint32 numpy array for
    numpy input, an int64 device tensor for torch device tensors."""
    A = arrays(x, device)
    p = A.xyz(x, y, z)
    cfg = _ransac_config(distance_threshold, max_iterations, probability, min_inliers, refine_model)
    idx = A.index(indices)
    m = A.n if idx is None else len(idx)
    inliers = A.index_out(m)
    r = capi.FdmRansacResult()
    _ck(capi.load().fdm_cloud_segment_plane(A.n, *p, A.on_device, A.ptr(idx), m, C.byref(cfg), A.device, A.ptr(inliers),
                                            C.byref(r)))
    return _ransac_result(A, r, inliers)


def segment_multiple_planes(x, y, z, distance_threshold=0.1, max_iterations=1000, probability=0.99, min_inliers=3,
                            refine_model=True, max_planes=5, min_fitness=0.1, device=0):
    """nanopcl::segmentation::segmentMultiplePlanes: planes are taken one after the other, each from the points the
    earlier ones left, until max_planes, fewer than 3 points, or a result without success or below min_fitness.
    Returns a list of RansacResult."""
    A = arrays(x, device)
    p = A.xyz(x, y, z)
    cfg = _ransac_config(distance_threshold, max_iterations, probability, min_inliers, refine_model)
    inliers = A.index_out(A.n)
    res = (capi.FdmRansacResult * max(int(max_planes), 1))()
    count = C.c_uint64(0)
    _ck(capi.load().fdm_cloud_segment_planes(A.n, *p, A.on_device, C.byref(cfg), int(max_planes), float(min_fitness),
                                             A.device, A.ptr(inliers), res, C.byref(count)))
    out, at = [], 0
    for k in range(int(count.value)):
        out.append(_ransac_result(A, res[k], inliers[at:]))
        at += int(res[k].n_inliers)
    return out


def segment_last_stats():
    """What this thread's last segmentation call did: n_batches (launches of the scoring kernel), n_hypotheses,
    n_invalid_samples, batch (iterations per launch), ms (zeros unless fdm_cloud_debug_profile is on)."""
    return _last_stats(capi.FdmSegmentStats, "fdm_segment_last_stats")


# ---- Euclidean clustering (fdm_cloud_cluster: include/fdm_engine.h) ----
class ClusterResult:
    """nanopcl::segmentation::ClusterResult in CSR form: indices (every clustered point's index into the cloud, cluster
    after cluster), offsets (num_clusters + 1 boundaries), and labels (per list position 0 = noise, else cluster number
    + 1).  Kept clusters come in descending size, equal sizes by their smallest list position; inside a cluster the list
    positions ascend.  uint32 numpy arrays for numpy input, int64 device tensors for torch device tensors."""

    def __init__(self, indices, offsets, labels):
        self.indices, self.offsets, self.labels = indices, offsets, labels

    @property
    def num_clusters(self):
        return max(len(self.offsets) - 1, 0)

    def __len__(self):
        return self.num_clusters

    @property
    def total_clustered_points(self):
        return len(self.indices)

    def cluster_size(self, i):
        return int(self.offsets[i + 1]) - int(self.offsets[i])

    def cluster_indices(self, i):
        """ClusterResult::clusterIndices(i): a view, no copy."""
        return self.indices[int(self.offsets[i]):int(self.offsets[i + 1])]

    def cluster_sizes(self):
        return self.offsets[1:] - self.offsets[:-1]

    def noise_indices(self, total):
        """ClusterResult::noiseIndices(total_points): the indices 0 .. total - 1 in no cluster, ascending."""
        return complement(self.indices, total)

    def __repr__(self):
        return f"ClusterResult(num_clusters={self.num_clusters}, total_clustered_points={self.total_clustered_points})"


def euclidean_cluster(x, y, z, indices=None, tolerance=0.5, min_size=10, max_size=100000, device=0):
    """nanopcl::segmentation::euclideanCluster on the device over the whole cloud or over `indices` (the values written
    are then the list's entries, i.e. indices into the cloud; a duplicate entry counts as two points).  Returns a
    ClusterResult; the relation and the order are stated in include/fdm_engine.h."""
    A = arrays(x, device)
    p = A.xyz(x, y, z)
    cfg = capi.FdmClusterConfig(float(np.float32(tolerance)), int(min_size), int(max_size))
    idx = A.index(indices)
    m = A.n if idx is None else len(idx)
    out, offsets, labels = A.index_out(m), A.index_out(m + 1), A.index_out(m)
    count = C.c_uint64(0)
    _ck(capi.load().fdm_cloud_cluster(A.n, *p, A.on_device, A.ptr(idx), m, C.byref(cfg), A.device, A.ptr(out),
                                      A.ptr(offsets), A.ptr(labels), C.byref(count)))
    k = int(count.value)
    off = A.take(offsets, k + 1)
    return ClusterResult(A.take(out, int(off[k])), off, A.take(labels, m))


def apply_cluster_labels(result, total, semantic_class=0):
    """nanopcl::segmentation::applyClusterLabels: the uint32 Label channel of a cloud of `total` points,
    (semantic_class << 16) | uint16(cluster number + 1) for a clustered point — the instance id truncated to 16 bits as
    in the reference — and (semantic_class << 16) for noise.  A numpy array."""
    sem = np.uint32((int(semantic_class) & 0xFFFF) << 16)
    out = np.full(int(total), sem, dtype=np.uint32)
    ind, off = to_numpy(result.indices), to_numpy(result.offsets)
    if ind.size:
        sizes = np.diff(off.astype(np.int64))
        ids = (np.arange(sizes.size, dtype=np.int64) + 1) & 0xFFFF
        out[ind.astype(np.int64)] = sem | np.repeat(ids, sizes).astype(np.uint32)
    return out


def cluster_last_stats():
    """What this thread's last euclidean_cluster did: the counts of fdm_cluster_stats and ms (zeros unless
    fdm_cloud_debug_profile is on)."""
    return _last_stats(capi.FdmClusterStats, "fdm_cluster_last_stats")
