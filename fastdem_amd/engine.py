"""Thin Python handle over the C ABI (include/fdm_engine.h) — used by tests and bench.py.

Mirrors the reference call shapes:
  ElevationMap(width, height, resolution, frame)  -> Engine(width, height, resolution, cfg)
  FastDEM::integrate(cloud, T_base_sensor, T_world_base) -> Engine.integrate(...)
  ElevationMapping::update(cloud, robot_position)        -> Engine.update(...)
Transforms are 4x4 row-major numpy arrays here and are handed to the ABI column-major
(Eigen::Isometry3d::matrix().data()).
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import (FdmCloud2Layout, FdmCloudOut, FdmCloudView, FdmConfig, FdmDemConfig, FdmDemStats, FdmGeometry, FdmRasterStats, FdmScanStats,
                   FdmNormalStats, FdmSorStats, FdmTile)


class EngineError(RuntimeError):
    pass


def _ck(rc):
    if rc < 0:
        raise EngineError(f"fdm_engine error {rc}: {capi.load().fdm_last_error().decode()}")
    return rc


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _u32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _colmajor16(T):
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    return np.ascontiguousarray(T.T).reshape(16)  # column-major flattening


def _dptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


class HostArray:
    """A 1-D numpy array over pinned memory from the engine's pool (fdm_host_alloc): what the host
    entry points read IN PLACE instead of copying.  Returned to the pool when collected."""

    def __init__(self, n, dtype=np.float32):
        self._lib = capi.load()
        dt = np.dtype(dtype)
        self._p = self._lib.fdm_host_alloc(max(int(n) * dt.itemsize, 1))
        if not self._p:
            raise MemoryError("fdm_host_alloc failed")
        buf = (C.c_char * (int(n) * dt.itemsize)).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dt, count=int(n))
        self.pinned = bool(self._lib.fdm_host_is_pinned(self._p))

    def __del__(self):
        if getattr(self, "_p", None):
            self.array = None
            self._lib.fdm_host_free(self._p)
            self._p = None


def host_array(values, dtype=np.float32):
    """Copy `values` into a pooled pinned array; keep the returned HostArray alive while `.array` is used."""
    v = np.ascontiguousarray(values, dtype=dtype).reshape(-1)
    h = HostArray(v.size, dtype)
    h.array[:] = v
    return h


def write_png(path, rgba):
    """uint8[height, width, 4] -> an 8-bit RGBA PNG, filter 0 on every scanline, through the standard library's zlib."""
    import struct
    import zlib
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    assert rgba.ndim == 3 and rgba.shape[2] == 4 and rgba.shape[0] > 0 and rgba.shape[1] > 0, rgba.shape
    h, w = rgba.shape[:2]
    lines = np.zeros((h, 1 + 4 * w), dtype=np.uint8)  # column 0: the filter type
    lines[:, 1:] = rgba.reshape(h, 4 * w)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(lines.tobytes(), 6)) + chunk(b"IEND", b""))


def _is_torch(a):
    return hasattr(a, "data_ptr")


def _raster_method(method):
    return capi.RASTER_METHOD[method] if isinstance(method, str) else int(method)


class Engine:
    # engine options (fdm_engine_set_option) every new Engine receives right after creation; the GPU test
    # suite uses it to run each test on both scan pipelines (tests/conftest.py)
    default_options = {}

    def __init__(self, width, height, resolution, cfg=None, position=(0.0, 0.0), tile=None,
                 device=0):
        self._lib = capi.load()
        self.cfg = cfg if cfg is not None else capi.default_config()
        g = FdmGeometry()
        # ElevationMap::setGeometry(float,float,float) promotes float -> double
        # (elevation_map.hpp:112-116): 0.1f becomes 0.100000001490116...
        g.length_x = float(np.float32(width))
        g.length_y = float(np.float32(height))
        g.resolution = float(np.float32(resolution))
        g.position_x, g.position_y = float(position[0]), float(position[1])
        self._tile = None
        tp = None
        if tile is not None:
            self._tile = FdmTile(*[int(v) for v in tile])
            tp = C.byref(self._tile)
        h = C.c_void_p()
        _ck(self._lib.fdm_engine_create(C.byref(g), C.byref(self.cfg), tp, int(device), C.byref(h)))
        self._h = h
        geo = self.geometry()
        self.rows, self.cols = geo.rows, geo.cols
        self.s_rows = self._tile.rows if self._tile else self.rows
        self.s_cols = self._tile.cols if self._tile else self.cols
        for key, value in type(self).default_options.items():
            self.set_option(key, value)

    @classmethod
    def _adopt(cls, handle):
        """An Engine over a handle the library created itself (fdm_engine_create_from_point_cloud): a map-only engine."""
        self = cls.__new__(cls)
        self._lib = capi.load()
        self.cfg = capi.default_config()
        self._tile = None
        self._h = handle
        try:
            geo = self.geometry()
            self.rows, self.cols = geo.rows, geo.cols
            self.s_rows, self.s_cols = self.rows, self.cols
            for key, value in cls.default_options.items():
                self.set_option(key, value)
        except Exception:
            self.close()  # (the handle is this object's alone: nobody else would destroy it)
            raise
        return self

    @classmethod
    def create_map(cls, width, height, resolution, position=(0.0, 0.0), device=0):
        """ElevationMap(width, height, resolution) alone (fdm_engine_create_map): the three basic layers, no estimator."""
        g = FdmGeometry()
        g.length_x, g.length_y = float(np.float32(width)), float(np.float32(height))
        g.resolution = float(np.float32(resolution))
        g.position_x, g.position_y = float(position[0]), float(position[1])
        h = C.c_void_p()
        _ck(capi.load().fdm_engine_create_map(C.byref(g), None, int(device), C.byref(h)))
        return cls._adopt(h)

    # -- lifetime --
    def close(self):
        if getattr(self, "_h", None):
            self._lib.fdm_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- configuration --
    def set_config(self, cfg):
        self.cfg = cfg
        _ck(self._lib.fdm_engine_set_config(self._h, C.byref(cfg)))

    def set_stream(self, stream_handle):
        _ck(self._lib.fdm_engine_set_stream(self._h, C.c_void_p(stream_handle)))

    def set_option(self, key, value):
        _ck(self._lib.fdm_engine_set_option(self._h, key.encode(), int(value)))

    # -- the hot path --
    def integrate(self, x, y, z, T_base_sensor, T_world_base, intensity=None, rgb=None,
                  sigma_z2=None):
        """Host arrays in, synchronous.  Returns (status, stats dict); status 0 == `true`."""
        x, y, z = _f32(x), _f32(y), _f32(z)
        a, c, v = _f32(intensity), _u32(rgb), _f32(sigma_z2)
        tbs, twb = _colmajor16(T_base_sensor), _colmajor16(T_world_base)
        st = FdmScanStats()
        rc = _ck(self._lib.fdm_engine_integrate(
            self._h, x.size, _ptr(x), _ptr(y), _ptr(z), _ptr(a), _ptr(c), _ptr(v),
            tbs.ctypes.data_as(C.POINTER(C.c_double)), twb.ctypes.data_as(C.POINTER(C.c_double)),
            C.byref(st)))
        return rc, st.as_dict()

    def integrate_points4(self, xyz1, T_base_sensor, T_world_base, intensity=None, rgb=None, sigma_z2=None):
        """The reference's own cloud layout: `xyz1` = n x 4 float32 records {x, y, z, 1} (nanopcl::PointCloud::points()),
        a C-contiguous HOST array (pinned memory is read in place).  Synchronous; returns (status, stats dict)."""
        import numpy as np
        p = xyz1 if isinstance(xyz1, np.ndarray) and xyz1.dtype == np.float32 and xyz1.flags["C_CONTIGUOUS"] \
            else np.ascontiguousarray(xyz1, dtype=np.float32)
        assert p.ndim == 2 and p.shape[1] == 4, p.shape
        a, c, v = _f32(intensity), _u32(rgb), _f32(sigma_z2)
        tbs, twb = _colmajor16(T_base_sensor), _colmajor16(T_world_base)
        st = FdmScanStats()
        rc = _ck(self._lib.fdm_engine_integrate_points4(
            self._h, p.shape[0], p.ctypes.data if p.shape[0] else None, _ptr(a), _ptr(c), _ptr(v),
            tbs.ctypes.data_as(C.POINTER(C.c_double)), twb.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
        return rc, st.as_dict()

    def wait_torch(self):
        """Order the engine's stream behind torch's current stream (an event + hipStreamWaitEvent): tensors
        produced by asynchronous torch work (copy_, kernels, NCCL results) are complete before the engine
        reads them.  The tensor-taking enqueue-only entry points call this themselves."""
        import torch
        # torch's stream idle: everything it produced is complete, nothing to order behind (a stream query is ~1 us; an
        # event record + a cross-stream wait are two more commands per call)
        if torch.cuda.current_stream().query():
            return
        if getattr(self, "_ev_in", None) is None:
            self._ev_in = torch.cuda.Event()
        self._ev_in.record()
        _ck(self._lib.fdm_engine_wait_event(self._h, C.c_void_p(self._ev_in.cuda_event)))

    def torch_wait(self):
        """Order torch's current stream behind the engine: launches a held-back map update, then makes
        torch's stream wait for everything the engine has enqueued (the map is current, the input arrays
        of every enqueued scan are free)."""
        import torch
        if getattr(self, "_ev_out", None) is None:
            self._ev_out = torch.cuda.Event()
            self._ev_out.record()  # (creates the HIP event)
        _ck(self._lib.fdm_engine_record_event(self._h, C.c_void_p(self._ev_out.cuda_event)))
        torch.cuda.current_stream().wait_event(self._ev_out)

    def integrate_device(self, x, y, z, T_base_sensor, T_world_base, intensity=None, rgb=None,
                         sigma_z2=None):
        """torch device tensors in, enqueue only (no sync).  The engine's stream is ordered behind torch's
        current stream first; the tensors may be reused once the enqueued work has run (torch_wait(), sync())
        — the held-back map update does not read them."""
        self.wait_torch()
        tbs, twb = _colmajor16(T_base_sensor), _colmajor16(T_world_base)
        _ck(self._lib.fdm_engine_integrate_device(
            self._h, x.numel(), _dptr(x), _dptr(y), _dptr(z), _dptr(intensity), _dptr(rgb),
            _dptr(sigma_z2), tbs.ctypes.data_as(C.POINTER(C.c_double)),
            twb.ctypes.data_as(C.POINTER(C.c_double))))

    def integrate_async(self, x, y, z, T_base_sensor, T_world_base, intensity=None, rgb=None):
        """Host arrays (ideally pinned), enqueue-only: H2D copy + scan on the engine stream."""
        x, y, z = _f32(x), _f32(y), _f32(z)
        a, c = _f32(intensity), _u32(rgb)
        tbs, twb = _colmajor16(T_base_sensor), _colmajor16(T_world_base)
        _ck(self._lib.fdm_engine_integrate_async(
            self._h, x.size, _ptr(x), _ptr(y), _ptr(z), _ptr(a), _ptr(c), None,
            tbs.ctypes.data_as(C.POINTER(C.c_double)), twb.ctypes.data_as(C.POINTER(C.c_double))))

    def integrate_async_raw(self, n, hx, hy, hz, tbs16, twb16, hint=None, hrgb=None):
        """Raw host pointers + pre-flattened transforms: the minimum-overhead streaming call."""
        return self._lib.fdm_engine_integrate_async(self._h, n, hx, hy, hz, hint, hrgb, None, tbs16, twb16)

    def integrate_device_raw(self, n, dx, dy, dz, tbs16, twb16, dint=None, drgb=None, dvar=None):
        """Pre-flattened column-major transforms (ctypes double arrays) + raw device pointers:
        the minimum-overhead call used inside bench.py's timed loop."""
        return self._lib.fdm_engine_integrate_device(self._h, n, dx, dy, dz, dint, drgb, dvar,
                                                     tbs16, twb16)

    def integrate_device_batch(self, scans, count=None):
        """`scans`: a ctypes array of capi.FdmDeviceScan — `count` device-resident scans enqueued by ONE call
        across the language boundary."""
        return self._lib.fdm_engine_integrate_device_batch(self._h, len(scans) if count is None else count, scans)

    def integrate_host_batch(self, scans, count=None, wait=True):
        """`scans`: a ctypes array of capi.FdmDeviceScan whose pointers are HOST pointers (pinned: read in place; pageable:
        staged) — N consecutive integrate() calls in batch launches.  wait: (status, statistics) of the last scan."""
        st = FdmScanStats()
        rc = _ck(self._lib.fdm_engine_integrate_host_batch(self._h, len(scans) if count is None else count, scans,
                                                           C.byref(st) if wait else None))
        return (rc, st.as_dict()) if wait else rc

    def integrate_device_batch_timed(self, scans, count=None):
        """The same between timer_start() and timer_stop(): timer_ms() afterwards is the batch's device time."""
        return self._lib.fdm_engine_integrate_device_batch_timed(self._h, len(scans) if count is None else count, scans)

    # -- scan routing for spatially tiled global maps (fdm_route.hpp) --
    def route_scan(self, plan, x, y, z, T_base_sensor, T_world_base, send, counts, intensity=None, soa=False):
        """Partition this rank's slice (torch device tensors) by owner rank into `send` ([n, 4] float32 device
        tensor: x, y, z, intensity records; `soa`: per owner four channel blocks of pad4(count) floats, the buffer
        then needs n + 3 * world rows) and leave the per-owner counts + n_after_filter + n_in_map in
        `counts` (device int32 tensor of world + 2).  Enqueue-only."""
        self.wait_torch()
        tbs, twb = _colmajor16(T_base_sensor), _colmajor16(T_world_base)
        fn = self._lib.fdm_engine_route_scan_soa if soa else self._lib.fdm_engine_route_scan
        _ck(fn(
            self._h, C.byref(plan), x.numel(), _dptr(x), _dptr(y), _dptr(z), _dptr(intensity),
            tbs.ctypes.data_as(C.POINTER(C.c_double)), twb.ctypes.data_as(C.POINTER(C.c_double)),
            _dptr(send), _dptr(counts)))

    def integrate_points4_device(self, points4, n, T_base_sensor, T_world_base, has_intensity=True, any_in_map=True):
        """FastDEM::integrate of `n` received {x, y, z, intensity} records (device tensor).  Enqueue-only."""
        self.wait_torch()
        tbs, twb = _colmajor16(T_base_sensor), _colmajor16(T_world_base)
        _ck(self._lib.fdm_engine_integrate_points4_device(
            self._h, int(n), _dptr(points4) if n else None, int(bool(has_intensity)), int(bool(any_in_map)),
            tbs.ctypes.data_as(C.POINTER(C.c_double)), twb.ctypes.data_as(C.POINTER(C.c_double))))

    def integrate_soa4_device(self, share, n, T_base_sensor, T_world_base, has_intensity=True, any_in_map=True):
        """FastDEM::integrate of one routed share (route_scan(soa=True)): `share` = flat float32 device tensor holding
        x | y | z | intensity, pad4(n) floats each, read in place.  Enqueue-only."""
        self.wait_torch()
        tbs, twb = _colmajor16(T_base_sensor), _colmajor16(T_world_base)
        _ck(self._lib.fdm_engine_integrate_soa4_device(
            self._h, int(n), _dptr(share) if n else None, int(bool(has_intensity)), int(bool(any_in_map)),
            tbs.ctypes.data_as(C.POINTER(C.c_double)), twb.ctypes.data_as(C.POINTER(C.c_double))))

    def update(self, x, y, z, robot_xy=(0.0, 0.0), z_var=None, intensity=None, rgb=None):
        x, y, z = _f32(x), _f32(y), _f32(z)
        v, a, c = _f32(z_var), _f32(intensity), _u32(rgb)
        st = FdmScanStats()
        n = 0 if x is None else x.size
        _ck(self._lib.fdm_engine_update(self._h, n, _ptr(x), _ptr(y), _ptr(z), _ptr(v), _ptr(a),
                                        _ptr(c), float(robot_xy[0]), float(robot_xy[1]),
                                        C.byref(st)))
        return st.as_dict()

    def last_pipeline(self):
        """0 = per-cell scratch pipeline, 1 = per-tile record pools (large scans), -1 = no scan yet."""
        return self._lib.fdm_engine_last_pipeline(self._h)

    def last_batch(self):
        """Scans of the batch launch the last scan left in (0: it took the single-scan path)."""
        return self._lib.fdm_engine_last_batch(self._h)

    def timer_start(self):
        """Mark the start of a timed run of enqueue-only calls on the engine's stream."""
        _ck(self._lib.fdm_engine_timer_start(self._h))

    def timer_stop(self):
        """Launch the last scan's held-back update and mark the end."""
        _ck(self._lib.fdm_engine_timer_stop(self._h))

    def timer_ms(self):
        ms = C.c_float(0.0)
        _ck(self._lib.fdm_engine_timer_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def debug_batch_dirty(self):
        """(keys, aux words, zero-sign words) of the batch scratch that are not clean after a flush: (0, 0, 0)."""
        out = (C.c_uint64 * 3)()
        _ck(self._lib.fdm_engine_debug_batch_dirty(self._h, out))
        return tuple(int(v) for v in out)

    def batch_launches(self):
        """(small-scan batch launches, tile-batch launches) enqueued since the engine was created."""
        out = (C.c_uint64 * 2)()
        _ck(self._lib.fdm_engine_debug_batch_launches(self._h, out))
        return int(out[0]), int(out[1])

    def debug_last_post_kernel(self):
        """Name of the kernel the last stencil-stage call launched ("k_median_sel", "k_features_tiled<6, 7>", ...); "" if it
        returned before launching."""
        buf = C.create_string_buffer(128)
        _ck(self._lib.fdm_engine_debug_last_post_kernel(self._h, buf, len(buf)))
        return buf.value.decode()

    def debug_timeline(self, cap_blocks=1 << 16):
        """(option dbg_timeline=1) -> (ticks[n_blocks, 2] uint64 of the 100 MHz clock, n_update_blocks) of the
        last fused large-scan launch."""
        buf = np.zeros((cap_blocks, 2), dtype=np.uint64)
        nb, nu = C.c_uint32(0), C.c_uint32(0)
        _ck(self._lib.fdm_engine_debug_timeline(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), cap_blocks,
                                                C.byref(nb), C.byref(nu)))
        return buf[:nb.value], nu.value

    def flush(self):
        """Launch a held-back map update (no wait)."""
        _ck(self._lib.fdm_engine_flush(self._h))

    def stream(self):
        """hipStream_t of the engine as an int."""
        return self._lib.fdm_engine_stream(self._h)

    def update_device(self, x, y, z, robot_xy=(0.0, 0.0), z_var=None, intensity=None, rgb=None):
        """ElevationMapping::update on torch device tensors (map-frame cloud), enqueue only."""
        self.wait_torch()
        _ck(self._lib.fdm_engine_update_device(self._h, x.numel(), _dptr(x), _dptr(y), _dptr(z), _dptr(z_var),
                                               _dptr(intensity), _dptr(rgb), float(robot_xy[0]),
                                               float(robot_xy[1])))

    def sync(self):
        _ck(self._lib.fdm_engine_sync(self._h))

    def last_stats(self):
        st = FdmScanStats()
        rc = _ck(self._lib.fdm_engine_last_stats(self._h, C.byref(st)))
        return rc, st.as_dict()

    # -- grid --
    def move(self, x, y):
        _ck(self._lib.fdm_engine_move(self._h, float(x), float(y)))

    def geometry(self):
        g = FdmGeometry()
        _ck(self._lib.fdm_engine_get_geometry(self._h, C.byref(g)))
        return g

    def set_position(self, x, y):
        _ck(self._lib.fdm_engine_set_position(self._h, float(x), float(y)))

    def set_start_index(self, r, c):
        _ck(self._lib.fdm_engine_set_start_index(self._h, int(r), int(c)))

    # -- layers --
    def layers(self):
        n = _ck(self._lib.fdm_engine_num_layers(self._h))
        return [self._lib.fdm_engine_layer_name(self._h, i).decode() for i in range(n)]

    def exists(self, name):
        return bool(_ck(self._lib.fdm_engine_layer_exists(self._h, name.encode())))

    def add(self, name, value=float("nan")):
        _ck(self._lib.fdm_engine_layer_add(self._h, name.encode(), float(value)))

    def layer(self, name):
        """Download one layer as a (rows, cols) float32 array (Fortran order like MatrixXf)."""
        out = np.empty((self.s_rows, self.s_cols), dtype=np.float32, order="F")
        _ck(self._lib.fdm_engine_layer_download(self._h, name.encode(), _ptr(out), self.s_rows,
                                                self.s_cols))
        return out

    def set_layer(self, name, arr):
        a = np.asfortranarray(arr, dtype=np.float32)
        assert a.shape == (self.s_rows, self.s_cols)
        _ck(self._lib.fdm_engine_layer_upload(self._h, name.encode(), _ptr(a), self.s_rows,
                                              self.s_cols))

    def copy_layer_from(self, other, name):
        """Layer `name` of another engine (same device, same window) into this one, device to device."""
        _ck(self._lib.fdm_engine_layer_copy(self._h, other._h, name.encode()))

    def layer_device_ptr(self, name):
        return self._lib.fdm_engine_layer_device_ptr(self._h, name.encode())

    def clear(self, name=None):
        _ck(self._lib.fdm_engine_clear(self._h, None if name is None else name.encode()))

    def region_pack(self, r0, c0, nr, nc, names, dbuf_ptr):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        _ck(self._lib.fdm_engine_region_pack(self._h, r0, c0, nr, nc, arr, len(names),
                                             C.c_void_p(dbuf_ptr)))

    def region_unpack(self, r0, c0, nr, nc, names, dbuf_ptr):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        _ck(self._lib.fdm_engine_region_unpack(self._h, r0, c0, nr, nc, arr, len(names),
                                               C.c_void_p(dbuf_ptr)))

    # -- stencil post-processing --
    def apply_inpainting(self, max_iterations=3, min_valid_neighbors=2, inplace=False):
        _ck(self._lib.fdm_engine_apply_inpainting(self._h, int(max_iterations), int(min_valid_neighbors),
                                                  int(inplace)))

    def apply_spatial_smoothing(self, layer, kernel_size=3, min_valid_neighbors=5):
        _ck(self._lib.fdm_engine_apply_spatial_smoothing(self._h, layer.encode(), int(kernel_size),
                                                         int(min_valid_neighbors)))

    def apply_uncertainty_fusion(self, enabled=True, search_radius=0.15, spatial_sigma=0.05,
                                 quantile_lower=0.01, quantile_upper=0.99, min_valid_neighbors=3):
        cfg = capi.FdmFusionConfig(int(enabled), search_radius, spatial_sigma, quantile_lower,
                                   quantile_upper, int(min_valid_neighbors))
        _ck(self._lib.fdm_engine_apply_uncertainty_fusion(self._h, C.byref(cfg)))

    def apply_feature_extraction(self, analysis_radius=0.3, min_valid_neighbors=4,
                                 step_lower_percentile=0.05, step_upper_percentile=0.95):
        _ck(self._lib.fdm_engine_apply_feature_extraction(self._h, analysis_radius, int(min_valid_neighbors),
                                                          step_lower_percentile, step_upper_percentile))

    # -- ingest --
    @staticmethod
    def cloud2_layout(point_step, x, y, z, intensity=-1, intensity_type=7, rgb=-1):
        return FdmCloud2Layout(int(point_step), int(x), int(y), int(z), int(intensity),
                               int(intensity_type), int(rgb))

    def ingest_cloud2(self, blob, n_points, layout, on_device_ptr=None):
        """nanopcl::from(PointCloud2): decode a host byte blob (or one already in HBM, `on_device_ptr`) into SoA
        channels in HBM.  Returns dict of numpy copies of the kept points' channels (for tests)."""
        n = C.c_uint64(0)
        if on_device_ptr is not None:
            data, dev = C.c_void_p(on_device_ptr), 1
        else:
            b = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8))
            data, dev = _ptr(b), 0
        _ck(self._lib.fdm_engine_ingest_cloud2(self._h, data, dev, int(n_points), C.byref(layout),
                                               C.byref(n)))
        ptrs = [C.c_void_p() for _ in range(5)]
        m = C.c_uint64(0)
        _ck(self._lib.fdm_engine_ingested(self._h, *[C.byref(p) for p in ptrs], C.byref(m)))
        assert m.value == n.value
        import torch
        out = {}
        for name, p, dt in zip(("x", "y", "z", "intensity", "rgb"), ptrs,
                               (np.float32,) * 4 + (np.uint32,)):
            if not p.value or n.value == 0:
                out[name] = None if name in ("intensity", "rgb") and not p.value else np.empty(0, dt)
                continue
            h = np.empty(n.value, dtype=dt)
            hip = C.CDLL("libamdhip64.so")
            assert hip.hipMemcpy(_ptr(h), p, h.nbytes, 2) == 0
            out[name] = h
        del torch
        return out

    def integrate_cloud2(self, blob, n_points, layout, T_base_sensor, T_world_base, on_device_ptr=None):
        """from_impl + integrate in one call; blob = bytes-like (host) or a device pointer."""
        tbs, twb = _colmajor16(T_base_sensor), _colmajor16(T_world_base)
        st = FdmScanStats()
        if on_device_ptr is not None:
            data, dev = C.c_void_p(on_device_ptr), 1
        else:
            b = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8))
            data, dev = _ptr(b), 0
        rc = _ck(self._lib.fdm_engine_integrate_cloud2(
            self._h, data, dev, int(n_points), C.byref(layout),
            tbs.ctypes.data_as(C.POINTER(C.c_double)), twb.ctypes.data_as(C.POINTER(C.c_double)),
            C.byref(st)))
        return rc, st.as_dict()

    # -- static point clouds (fastdem/io/pcd_convert.hpp) --
    def from_point_cloud(self, x, y, z, intensity=None, rgb=None, method="max"):
        """fastdem::fromPointCloud(cloud, map, method): numpy arrays (staged) or torch device tensors (read in place).
        Synchronous.  Returns (status, {"n_points_used", "n_cells_written"}); status 0 = written, 1 = empty cloud,
        3 = no point landed in a cell (the map, its layer list included, is untouched)."""
        st = FdmRasterStats()
        m = _raster_method(method)
        if _is_torch(x):
            import torch
            torch.cuda.current_stream().synchronize()  # the call reads the tensors at once, on the engine's stream
            rc = _ck(self._lib.fdm_engine_from_point_cloud_device(
                self._h, x.numel(), _dptr(x), _dptr(y), _dptr(z), _dptr(intensity), _dptr(rgb), m, C.byref(st)))
        else:
            x, y, z = _f32(x), _f32(y), _f32(z)
            a, c = _f32(intensity), _u32(rgb)
            rc = _ck(self._lib.fdm_engine_from_point_cloud(self._h, x.size, _ptr(x), _ptr(y), _ptr(z), _ptr(a), _ptr(c),
                                                           m, C.byref(st)))
        return rc, {"n_points_used": int(st.n_points_used), "n_cells_written": int(st.n_cells_written)}

    def remove_floating_points(self, x, y, z, height_threshold=2.0, bin_size=0.0):
        """removeFloatingPoints(cloud, map, height_threshold, bin) on this map's geometry: the keep mask (bool[n], or a
        torch uint8 device tensor for device tensors).  bin_size 0 = the resolution.  The map is not touched."""
        n_kept = C.c_uint64(0)
        if _is_torch(x):
            import torch
            torch.cuda.current_stream().synchronize()
            keep = torch.zeros(x.numel(), dtype=torch.uint8, device=x.device)
            _ck(self._lib.fdm_engine_remove_floating_points(self._h, x.numel(), _dptr(x), _dptr(y), _dptr(z), 1,
                                                            float(height_threshold), float(bin_size), _dptr(keep),
                                                            C.byref(n_kept)))
            return keep
        x, y, z = _f32(x), _f32(y), _f32(z)
        keep = np.zeros(x.size, dtype=np.uint8)
        _ck(self._lib.fdm_engine_remove_floating_points(self._h, x.size, _ptr(x), _ptr(y), _ptr(z), 0,
                                                        float(height_threshold), float(bin_size), _ptr(keep),
                                                        C.byref(n_kept)))
        assert int(keep.sum()) == n_kept.value
        return keep.astype(bool)

    def last_raster_ms(self):
        """(ids, grouping, walk) device ms of the last from_point_cloud (enable_profile() first)."""
        ms = (C.c_float * 3)()
        _ck(self._lib.fdm_engine_last_raster_ms(self._h, ms))
        return tuple(float(v) for v in ms)

    def to_point_cloud(self):
        """fastdem::toPointCloud(map): dict x, y, z (float32), intensity (float32 or None), rgb (uint32 0x00RRGGBB or
        None) — one point per cell whose elevation is not NaN; a channel is None when no emitted cell has a value."""
        n, hi, hc = C.c_uint64(0), C.c_int32(0), C.c_int32(0)
        cap = self.rows * self.cols
        x, y, z, a = (np.empty(cap, dtype=np.float32) for _ in range(4))
        c = np.empty(cap, dtype=np.uint32)
        _ck(self._lib.fdm_engine_to_point_cloud(self._h, cap, _ptr(x), _ptr(y), _ptr(z), _ptr(a), _ptr(c), C.byref(n),
                                                C.byref(hi), C.byref(hc)))
        k = n.value
        return {"x": x[:k].copy(), "y": y[:k].copy(), "z": z[:k].copy(),
                "intensity": a[:k].copy() if hi.value else None, "rgb": c[:k].copy() if hc.value else None}

    def to_point_cloud_device(self):
        """The same with the channels left in HBM until the next call: (device pointers x, y, z, intensity, rgb; count;
        has_intensity; has_color)."""
        ptrs = [C.c_void_p() for _ in range(5)]
        n, hi, hc = C.c_uint64(0), C.c_int32(0), C.c_int32(0)
        _ck(self._lib.fdm_engine_to_point_cloud_device(self._h, *[C.byref(p) for p in ptrs], C.byref(n), C.byref(hi),
                                                       C.byref(hc)))
        return [p.value for p in ptrs], n.value, bool(hi.value), bool(hc.value)

    def to_pcd(self):
        """The binary data section of nanopcl::io::savePCD(toPointCloud(map)), packed on the device: (bytes, n_points,
        has_intensity, has_color).  fastdem_amd.pcd.write_header gives the header that goes in front."""
        cap = self.rows * self.cols * 20
        buf = np.empty(max(cap, 1), dtype=np.uint8)
        nb, n, hi, hc = C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_int32(0)
        rc = _ck(self._lib.fdm_engine_to_pcd(self._h, _ptr(buf), cap, C.byref(nb), C.byref(n), C.byref(hi), C.byref(hc)))
        assert rc == 0, rc
        return buf[:nb.value].tobytes(), n.value, bool(hi.value), bool(hc.value)

    # -- egress --
    def pack_cloud(self, elevation_layer="elevation", sub=None, names_cap=4096):
        """toPointCloud2Impl on the device: (fields, point_step, data[n_points, n_fields] float32).
        names_cap: bytes of the buffer the field names are received in."""
        r0, c0, nr, nc = sub if sub is not None else (0, 0, -1, -1)
        n, step = C.c_uint64(0), C.c_uint32(0)
        names = C.create_string_buffer(names_cap)
        name = elevation_layer.encode()
        _ck(self._lib.fdm_engine_pack_cloud(self._h, name, r0, c0, nr, nc, None, 0, C.byref(n),
                                            C.byref(step), names, names_cap))
        fields = names.value.decode().split("\n")
        data = np.empty((n.value, len(fields)), dtype=np.float32)
        if n.value:
            _ck(self._lib.fdm_engine_pack_cloud(self._h, name, r0, c0, nr, nc, _ptr(data), data.nbytes,
                                                C.byref(n), C.byref(step), None, 0))
        return fields, step.value, data

    def pack_cloud_device(self, elevation_layer="elevation", sub=None):
        """Records stay in HBM: (device pointer, n_points, point_step)."""
        r0, c0, nr, nc = sub if sub is not None else (0, 0, -1, -1)
        n, step, d = C.c_uint64(0), C.c_uint32(0), C.c_void_p()
        _ck(self._lib.fdm_engine_pack_cloud_device(self._h, elevation_layer.encode(), r0, c0, nr, nc,
                                                   C.byref(d), C.byref(n), C.byref(step)))
        return d.value, n.value, step.value

    # -- layer images (fastdem::io::savePng's pixels) --
    @staticmethod
    def _image_config(normalize, colormap, align_to_world, fixed):
        def enum(table, v):
            return table[v] if isinstance(v, str) else int(v)
        return capi.FdmImageConfig(enum(capi.NORMALIZE, normalize), enum(capi.COLORMAP, colormap),
                                   int(bool(align_to_world)), float(fixed[0]), float(fixed[1]))

    def render_layer(self, layer, normalize="percentile_1_99", colormap="viridis", align_to_world=True,
                     fixed=(-2.0, 2.0)):
        """One layer as savePng colours it, computed on the device: (rgba uint8[rows, cols, 4], (vmin, vmax))."""
        cfg = self._image_config(normalize, colormap, align_to_world, fixed)
        w, h = C.c_int32(0), C.c_int32(0)
        name = layer.encode()
        _ck(self._lib.fdm_engine_render_layer(self._h, name, C.byref(cfg), None, 0, C.byref(w), C.byref(h), None))
        rgba = np.empty((h.value, w.value, 4), dtype=np.uint8)
        rng = (C.c_float * 2)()
        _ck(self._lib.fdm_engine_render_layer(self._h, name, C.byref(cfg), _ptr(rgba), rgba.nbytes, C.byref(w),
                                              C.byref(h), rng))
        return rgba, (np.float32(rng[0]), np.float32(rng[1]))

    def render_layer_device(self, layer, normalize="percentile_1_99", colormap="viridis", align_to_world=True,
                            fixed=(-2.0, 2.0), want_range=True):
        """The image stays in HBM until the next render: (device pointer, width, height, (vmin, vmax) or None)."""
        cfg = self._image_config(normalize, colormap, align_to_world, fixed)
        w, h, d = C.c_int32(0), C.c_int32(0), C.c_void_p()
        rng = (C.c_float * 2)()
        _ck(self._lib.fdm_engine_render_layer_device(self._h, layer.encode(), C.byref(cfg), C.byref(d), C.byref(w),
                                                     C.byref(h), rng if want_range else None))
        return d.value, w.value, h.value, ((np.float32(rng[0]), np.float32(rng[1])) if want_range else None)

    def save_png(self, path, layer, **image):
        """fastdem::io::savePng: render `layer` (keywords as render_layer) and write it as an 8-bit RGBA PNG."""
        rgba, _ = self.render_layer(layer, **image)
        write_png(path, rgba)

    # -- raycasting stage --
    def apply_raycasting(self, x, y, z, sensor_origin, rc=None):
        """fastdem::applyRaycasting(map, scan, sensor_origin, config); host arrays, sync.
        rc: capi.FdmRaycastConfig, None = the raycasting fields of the engine config."""
        x, y, z = _f32(x), _f32(y), _f32(z)
        o = (C.c_float * 3)(*[float(v) for v in sensor_origin])
        _ck(self._lib.fdm_engine_apply_raycasting(self._h, x.size, _ptr(x), _ptr(y), _ptr(z), o,
                                                  None if rc is None else C.byref(rc)))

    def apply_raycasting_device(self, x, y, z, sensor_origin, rc=None):
        o = (C.c_float * 3)(*[float(v) for v in sensor_origin])
        _ck(self._lib.fdm_engine_apply_raycasting_device(self._h, x.numel(), _dptr(x), _dptr(y),
                                                         _dptr(z), o,
                                                         None if rc is None else C.byref(rc)))

    def voxel_any(self, x, y, z, voxel_size):
        """filters::voxelGrid(cloud, voxel_size, VoxelMode::ANY): original indices, output order."""
        x, y, z = _f32(x), _f32(y), _f32(z)
        out = np.empty(max(x.size, 1), dtype=np.uint32)
        n = C.c_uint64(0)
        _ck(self._lib.fdm_engine_voxel_any(self._h, x.size, _ptr(x), _ptr(y), _ptr(z),
                                           float(voxel_size), _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def last_ray_ms(self):
        ms = C.c_float(0)
        _ck(self._lib.fdm_engine_last_ray_ms(self._h, C.byref(ms)))
        return float(ms.value)

    # -- scan callbacks --
    def capture(self, preprocessed=True, rasterized=True):
        _ck(self._lib.fdm_engine_capture(self._h, int(preprocessed), int(rasterized)))

    def last_preprocessed(self, cap):
        a = [np.empty(cap, dtype=np.float32) for _ in range(4)]
        n = C.c_uint64(0)
        _ck(self._lib.fdm_engine_last_preprocessed(self._h, cap, *[_ptr(v) for v in a], C.byref(n)))
        return [v[:n.value] for v in a]

    def last_preprocessed_cov(self, cap):
        """(n, 3, 3) covariance channel of the preprocessed cloud (capture(preprocessed=2))."""
        a = np.empty((cap, 9), dtype=np.float32)
        n = C.c_uint64(0)
        _ck(self._lib.fdm_engine_last_preprocessed_cov(self._h, cap, _ptr(a), C.byref(n)))
        return a[:n.value].reshape(-1, 3, 3).transpose(0, 2, 1)  # column-major 3x3 per point

    def last_rasterized(self, cap):
        a = [np.empty(cap, dtype=np.float32) for _ in range(3)]
        n = C.c_uint64(0)
        _ck(self._lib.fdm_engine_last_rasterized(self._h, cap, *[_ptr(v) for v in a], C.byref(n)))
        return [v[:n.value] for v in a]

    # -- instrumentation --
    def enable_cell_ids(self, on=True):
        _ck(self._lib.fdm_engine_enable_cell_ids(self._h, int(on)))

    def last_cell_ids(self, n):
        out = np.empty(n, dtype=np.int32)
        _ck(self._lib.fdm_engine_last_cell_ids(self._h, _ptr(out), n))
        return out

    def enable_profile(self, on=True):
        _ck(self._lib.fdm_engine_enable_profile(self._h, int(on)))

    def last_kernel_ms(self):
        ms = (C.c_float * 2)()
        _ck(self._lib.fdm_engine_last_kernel_ms(self._h, ms))
        return float(ms[0]), float(ms[1])


def from_point_cloud(x, y, z, resolution, intensity=None, rgb=None, method="max", device=0):
    """fastdem::fromPointCloud(cloud, resolution, method): a map-only Engine sized to the cloud's x / y bounding box
    (found on the device) with the cloud rasterized into it; None for an empty cloud.  numpy arrays or torch device
    tensors.  A cloud without a finite, positive extent (every x or y NaN, an infinite coordinate) raises EngineError."""
    lib = capi.load()
    h, st = C.c_void_p(), FdmRasterStats()
    m = _raster_method(method)
    if _is_torch(x):
        import torch
        torch.cuda.current_stream().synchronize()
        n, on_device = x.numel(), 1
        args = [_dptr(v) for v in (x, y, z, intensity, rgb)]
    else:
        x, y, z = _f32(x), _f32(y), _f32(z)
        keep = (x, y, z, _f32(intensity), _u32(rgb))
        n, on_device = x.size, 0
        args = [_ptr(v) for v in keep]
    rc = _ck(lib.fdm_engine_create_from_point_cloud(n, *args, on_device, float(np.float32(resolution)), m, int(device),
                                                    C.byref(h), C.byref(st)))
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


def sor_last_stats():
    """What this thread's last outlier removal did: n_queries, n_fallback (queries the brute-force queue took), grid_x,
    grid_y, voxel, ms (grid build, search, fallback queue, statistics)."""
    st = FdmSorStats()
    _ck(capi.load().fdm_sor_last_stats(C.byref(st)))
    return {"n_queries": int(st.n_queries), "n_fallback": int(st.n_fallback), "grid_x": int(st.grid_x),
            "grid_y": int(st.grid_y), "voxel": float(st.voxel), "ms": tuple(float(v) for v in st.ms)}


def statistical_outlier_removal(x, y, z, k=10, std_mul=1.0, device=0, return_details=False):
    """nanopcl::filters::statisticalOutlierRemoval(cloud, k, std_mul) as a keep mask over the input points: bool[n] for
    numpy arrays, a torch uint8 device tensor for torch device tensors.  return_details: (keep, mean_dist, threshold)
    with mean_dist the per-point mean distance to its k nearest neighbours (float32) and threshold a np.float32."""
    lib = capi.load()
    thr, n_kept = C.c_float(0.0), C.c_uint64(0)
    if _is_torch(x):
        import torch
        torch.cuda.current_stream().synchronize()
        n = x.numel()
        keep = torch.zeros(n, dtype=torch.uint8, device=x.device)
        mean = torch.zeros(n, dtype=torch.float32, device=x.device)
        _ck(lib.fdm_statistical_outlier_removal(n, _dptr(x), _dptr(y), _dptr(z), 1, int(k), float(np.float32(std_mul)),
                                                int(device), _dptr(keep), _dptr(mean), C.byref(thr), C.byref(n_kept)))
    else:
        x, y, z = _f32(x), _f32(y), _f32(z)
        n = x.size
        keep8 = np.zeros(n, dtype=np.uint8)
        mean = np.zeros(n, dtype=np.float32)
        _ck(lib.fdm_statistical_outlier_removal(n, _ptr(x), _ptr(y), _ptr(z), 0, int(k), float(np.float32(std_mul)),
                                                int(device), _ptr(keep8), _ptr(mean), C.byref(thr), C.byref(n_kept)))
        assert int(keep8.sum()) == n_kept.value
        keep = keep8.astype(bool)
    return (keep, mean, np.float32(thr.value)) if return_details else keep


def build_dem(x, y, z, intensity=None, rgb=None, config=None, device=0, return_stats=False):
    """fastdem::buildDEM(cloud, config): outlier removal, floating-point removal, rasterization and inpainting on the
    device.  Returns a map-only Engine, or None where the reference returns an uninitialised map (an empty cloud, a
    cloud the outlier removal empties).  numpy arrays or torch device tensors.  return_stats: (engine, dict of
    fdm_dem_stats)."""
    lib = capi.load()
    cfg = (config if config is not None else DEMConfig()).as_struct()
    h, st = C.c_void_p(), FdmDemStats()
    if _is_torch(x):
        import torch
        torch.cuda.current_stream().synchronize()
        n, on_device = x.numel(), 1
        args = [_dptr(v) for v in (x, y, z, intensity, rgb)]
    else:
        x, y, z = _f32(x), _f32(y), _f32(z)
        keep = (x, y, z, _f32(intensity), _u32(rgb))
        n, on_device = x.size, 0
        args = [_ptr(v) for v in keep]
    rc = _ck(lib.fdm_engine_build_dem(n, *args, on_device, C.byref(cfg), int(device), C.byref(h), C.byref(st)))
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
    torch_in = _is_torch(x)
    if normals is not None and not isinstance(normals, (tuple, list)):
        normals = tuple(normals[:, k] for k in range(3))       # an (n, 3) array
    if torch_in:
        import torch
        torch.cuda.current_stream(x.device).synchronize()
        device = x.device.index if x.device.index is not None else torch.cuda.current_device()  # where the tensors live
        n = x.numel()
        given = {"x": x, "y": y, "z": z, "intensity": intensity, "rgb": rgb, "cov9": cov}
        for k, v in zip(("nx", "ny", "nz"), normals or (None,) * 3):
            given[k] = v
        given = {k: (None if v is None else v.contiguous()) for k, v in given.items()}
        outs = {k: torch.empty((n, 9) if k == "cov9" else n, dtype=v.dtype, device=x.device)
                for k, v in given.items() if v is not None}
        outs["idx"] = torch.empty(n, dtype=torch.int32, device=x.device)
        ptr = _dptr
    else:
        x, y, z = _f32(x).reshape(-1), _f32(y).reshape(-1), _f32(z).reshape(-1)
        n = x.size
        given = {"x": x, "y": y, "z": z, "intensity": _f32(intensity), "rgb": _u32(rgb),
                 "cov9": None if cov is None else _f32(cov).reshape(n, 9)}
        for k, v in zip(("nx", "ny", "nz"), normals or (None,) * 3):
            given[k] = _f32(v)
        outs = {k: np.empty((n, 9) if k == "cov9" else n, dtype=v.dtype) for k, v in given.items() if v is not None}
        outs["idx"] = np.empty(n, dtype=np.uint32)
        ptr = _ptr
    view = FdmCloudView(**{k: ptr(v) for k, v in given.items()})
    out = FdmCloudOut(**{k: ptr(v) for k, v in outs.items()})
    n_out = C.c_uint64(0)
    size = float(np.float32(size))
    if mode is None:
        _ck(lib.fdm_cloud_grid_max_z(n, C.byref(view), int(torch_in), size, int(order), int(device), C.byref(out),
                                     C.byref(n_out)))
    else:
        m = capi.VOXEL_MODE[mode.lower()] if isinstance(mode, str) else int(mode)
        _ck(lib.fdm_cloud_voxel_grid(n, C.byref(view), int(torch_in), size, m, int(order), int(device), C.byref(out),
                                     C.byref(n_out)))
    k = int(n_out.value)
    res = {name: v[:k] for name, v in outs.items()}
    if "nx" in res:
        res["normals"] = (res.pop("nx"), res.pop("ny"), res.pop("nz"))
    if "cov9" in res:
        res["cov"] = res.pop("cov9")
    idx = res.pop("idx")
    if return_index:
        res["idx"] = (idx.long() & 0xFFFFFFFF) if torch_in else idx
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
    st = FdmNormalStats()
    _ck(capi.load().fdm_normals_last_stats(C.byref(st)))
    return {"n_queries": int(st.n_queries), "n_fallback": int(st.n_fallback), "n_invalid": int(st.n_invalid),
            "grid_x": int(st.grid_x), "grid_y": int(st.grid_y), "voxel": float(st.voxel),
            "ms": tuple(float(v) for v in st.ms)}


def estimate_normals(x, y, z, k=20, viewpoint=(0.0, 0.0, 0.0), covariances=False, device=0, return_stats=False):
    """nanopcl::geometry::estimateNormals(cloud, k, viewpoint) on the device, or estimateNormalsCovariances with
    covariances=True: per point the PCA of its k nearest points (itself included), the normal turned towards the
    viewpoint, the covariance regularised for GICP to eigenvalues (1e-3, 1, 1).  numpy arrays in, numpy arrays out; torch
    device tensors in, device tensors out.  Returns normals[n, 3], or (normals, cov[n, 3, 3]) with covariances; points
    with fewer than 3 neighbours or a degenerate neighbourhood get a zero normal and the identity.  return_stats appends
    normals_last_stats().  device: the ordinal numpy input runs on; torch tensors run on the device they live on."""
    lib = capi.load()
    vp = (C.c_float * 3)(*[float(np.float32(v)) for v in viewpoint])
    n_invalid = C.c_uint64(0)
    if _is_torch(x):
        import torch
        torch.cuda.current_stream(x.device).synchronize()
        device = x.device.index if x.device.index is not None else torch.cuda.current_device()
        x, y, z = (v.contiguous() for v in (x, y, z))
        n = x.numel()
        soa = torch.empty((3, n), dtype=torch.float32, device=x.device)
        cov9 = torch.empty((n, 9), dtype=torch.float32, device=x.device) if covariances else None
        _ck(lib.fdm_cloud_estimate_normals(n, _dptr(x), _dptr(y), _dptr(z), 1, int(k), vp, int(device), _dptr(soa[0]),
                                           _dptr(soa[1]), _dptr(soa[2]), _dptr(cov9), C.byref(n_invalid)))
        normals = soa.t().contiguous()
        cov = cov9.view(n, 3, 3).transpose(1, 2).contiguous() if covariances else None   # column-major -> [row][column]
    else:
        x, y, z = _f32(x).reshape(-1), _f32(y).reshape(-1), _f32(z).reshape(-1)
        n = x.size
        soa = np.empty((3, n), dtype=np.float32)
        cov9 = np.empty((n, 9), dtype=np.float32) if covariances else None
        _ck(lib.fdm_cloud_estimate_normals(n, _ptr(x), _ptr(y), _ptr(z), 0, int(k), vp, int(device), _ptr(soa[0]),
                                           _ptr(soa[1]), _ptr(soa[2]), _ptr(cov9), C.byref(n_invalid)))
        normals = np.ascontiguousarray(soa.T)
        cov = np.ascontiguousarray(cov9.reshape(n, 3, 3).transpose(0, 2, 1)) if covariances else None
    out = (normals, cov) if covariances else (normals,)
    if return_stats:
        out = out + (normals_last_stats(),)
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


def _cov_colmajor(cov, n):
    """n covariances indexed [row][column] (a NumPy array or a torch tensor, or None) as (n, 3, 3) column-major, contiguous."""
    if cov is None:
        return None
    if _is_torch(cov):
        return cov.reshape(n, 3, 3).transpose(1, 2).contiguous()
    return np.ascontiguousarray(cov.reshape(n, 3, 3).transpose(0, 2, 1))


def _registration_result(res):
    """RegistrationResult of an FdmRegistrationResult."""
    T = np.array(res.transform, dtype=np.float64).reshape(4, 4).T.copy()
    cov = np.array(res.covariance, dtype=np.float64).reshape(6, 6) if res.has_covariance else None
    return RegistrationResult(T, float(res.fitness), float(res.rmse), int(res.iterations), bool(res.converged), cov)


def _linearized(entry, n, like, return_correspondences):
    """The outputs of one linearize entry: makes H, b, error, num_inliers and (asked for) corr — n int32 where the clouds
    live: on the device of the tensor `like`, or in a NumPy array for `like` None —, calls entry(H, b, error, num_inliers,
    corr) and returns the result dict."""
    H, b = (C.c_double * 21)(), (C.c_double * 6)()
    err, cnt = C.c_double(0.0), C.c_uint64(0)
    corr = None
    if return_correspondences:
        if like is not None:
            import torch
            corr = torch.empty(n, dtype=torch.int32, device=like.device)
        else:
            corr = np.empty(n, dtype=np.int32)
    _ck(entry(H, b, C.byref(err), C.byref(cnt), (_ptr if like is None else _dptr)(corr)))
    Hu = np.array(H, dtype=np.float64)
    full = np.zeros((6, 6))
    full[np.triu_indices(6)] = Hu
    full = full + np.triu(full, 1).T
    out = {"H": full, "H_upper": Hu, "b": np.array(b, dtype=np.float64), "error": float(err.value),
           "num_inliers": int(cnt.value)}
    if return_correspondences:
        out["corr"] = corr
    return out


def _register_clouds(source, target, target_normals, source_cov, target_cov):
    """(FdmRegisterClouds, device or None, the arrays it points into) for numpy arrays or torch device tensors."""
    sx, sy, sz = source
    tx, ty, tz = target
    torch_in = _is_torch(sx)
    if torch_in:
        import torch
        torch.cuda.current_stream(sx.device).synchronize()
        device = sx.device.index if sx.device.index is not None else torch.cuda.current_device()

        def prep(v):
            if v is None:
                return None
            if not _is_torch(v) or v.dtype != torch.float32 or v.device != sx.device:
                raise TypeError("registration takes float32 tensors that all live on the source's device "
                                "(or NumPy arrays throughout)")
            return v.contiguous()
        ptr, size = _dptr, lambda v: v.numel()                                     # noqa: E731
    else:
        device = None

        def prep(v):
            if _is_torch(v):
                raise TypeError("registration takes NumPy arrays throughout or torch device tensors throughout")
            return None if v is None else _f32(v).reshape(-1)
        ptr, size = _ptr, lambda v: v.size                                         # noqa: E731
    if target_normals is not None and not isinstance(target_normals, (tuple, list)):
        target_normals = tuple(target_normals[:, k] for k in range(3))              # an (n, 3) array
    keep = [prep(v) for v in (sx, sy, sz, tx, ty, tz)] + [prep(v) for v in (target_normals or (None,) * 3)]
    ns, nt = size(keep[0]), size(keep[3])
    keep += [_cov_colmajor(prep(source_cov), ns), _cov_colmajor(prep(target_cov), nt)]
    p = [ptr(v) for v in keep]
    clouds = capi.FdmRegisterClouds(ns, p[0], p[1], p[2], p[9], nt, p[3], p[4], p[5], p[6], p[7], p[8], p[10],
                                    int(torch_in))
    return clouds, device, keep


def _guess16(T):
    return None if T is None else (C.c_double * 16)(*_colmajor16(T))


def _register(method, source, target, initial_guess, target_normals, source_cov, target_cov, device, settings):
    clouds, dev, keep = _register_clouds(source, target, target_normals, source_cov, target_cov)
    st = settings.pop("settings", None) or align_settings(**settings)
    res = capi.FdmRegistrationResult()
    _ck(capi.load().fdm_cloud_register(capi.REGISTER_METHOD[method], C.byref(clouds), _guess16(initial_guess),
                                       C.byref(st), int(device if dev is None else dev), C.byref(res)))
    del keep
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
    clouds, dev, keep = _register_clouds((sx, sy, sz), (tx, ty, tz), target_normals, source_cov, target_cov)
    st = settings.pop("settings", None) or align_settings(**settings)
    lib, number = capi.load(), capi.REGISTER_METHOD[method]
    return _linearized(lambda *out: lib.fdm_cloud_register_linearize(number, C.byref(clouds), _guess16(transform),
                                                                     C.byref(st), int(device if dev is None else dev), *out),
                       int(clouds.n_source), keep[0] if clouds.on_device else None, return_correspondences)


def register_last_stats():
    """What this thread's last registration call did: n_source, n_target, grid_x, grid_y, voxel (the target's search
    grid), ring_limit, linearizations, ms (grid build, regularisation, the linearizations summed; zeros unless
    fdm_cloud_debug_profile is on)."""
    st = capi.FdmRegisterStats()
    _ck(capi.load().fdm_register_last_stats(C.byref(st)))
    return {"n_source": int(st.n_source), "n_target": int(st.n_target), "grid_x": int(st.grid_x), "grid_y": int(st.grid_y),
            "voxel": float(st.voxel), "ring_limit": int(st.ring_limit), "linearizations": int(st.linearizations),
            "ms": tuple(float(v) for v in st.ms)}


# ---- voxelized GICP (fdm_voxel_map_* / fdm_cloud_register_vgicp: include/fdm_engine.h) ----
class VoxelMap:
    """nanopcl::registration::VoxelDistributionMap on the device: per-voxel means and covariances of a target cloud, built
    once and registered against any number of times (align_vgicp, linearize_vgicp).  x, y, z: NumPy arrays, or torch
    device tensors (the map then lives on their device).  Owns device memory until close() (or the end of a `with`)."""

    def __init__(self, x, y, z, resolution=1.0, covariance_epsilon=1e-3, device=0):
        self._h = None
        n, p, on_device, dev, keep, _ = _seg_cloud(x, y, z, device)
        h = C.c_void_p()
        _ck(capi.load().fdm_voxel_map_create(n, p[0], p[1], p[2], on_device, float(resolution),
                                             float(covariance_epsilon), int(dev), C.byref(h)))
        del keep
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
        out = {k: getattr(st, k) for k in ("resolution", "inv_resolution", "covariance_epsilon", "device", "n_points",
                                           "n_skipped", "num_voxels", "n_sparse", "max_count", "table_slots",
                                           "max_probe")}
        out["ms"] = tuple(float(v) for v in st.ms)
        return out

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


def _vgicp_source(sx, sy, sz, source_cov, device):
    """(n, pointers of x y z cov9, on_device, the arrays kept alive) of a NumPy or torch device source cloud."""
    n, p, on_device, _, keep, torch = _seg_cloud(sx, sy, sz, device)
    cov = None
    if source_cov is not None:
        if torch is not None and (not _is_torch(source_cov) or source_cov.device != keep[0].device):
            raise TypeError("registration takes float32 tensors that all live on the source's device "
                            "(or NumPy arrays throughout)")
        cov = _cov_colmajor(source_cov.float() if torch is not None else _f32(source_cov), n)
    return n, p + [(_dptr if on_device else _ptr)(cov)], on_device, keep + (cov,)


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
        n, p, on_device, keep = _vgicp_source(sx, sy, sz, source_cov, device)
        res = capi.FdmRegistrationResult()
        _ck(capi.load().fdm_cloud_register_vgicp(vmap._handle(), n, p[0], p[1], p[2], p[3], on_device,
                                                 _guess16(initial_guess), C.byref(st), C.byref(res)))
        del keep
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
        n, p, on_device, keep = _vgicp_source(sx, sy, sz, source_cov, device)
        lib = capi.load()
        return _linearized(lambda *out: lib.fdm_cloud_register_vgicp_linearize(vmap._handle(), n, p[0], p[1], p[2], p[3],
                                                                               on_device, _guess16(transform),
                                                                               C.byref(st), *out),
                           n, keep[0] if on_device else None, return_correspondences)
    finally:
        if mine:
            vmap.close()


# ---- cloud segmentation (fdm_cloud_segment_ground / _plane / _planes: include/fdm_engine.h) ----
def _seg_cloud(x, y, z, device):
    """(n, pointers of x y z, on_device, device, the arrays kept alive, torch module or None)."""
    if _is_torch(x):
        import torch
        torch.cuda.current_stream(x.device).synchronize()
        dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
        keep = tuple(v.contiguous().float() for v in (x, y, z))
        return keep[0].numel(), [_dptr(v) for v in keep], 1, dev, keep, torch
    keep = tuple(_f32(v).reshape(-1) for v in (x, y, z))
    return keep[0].size, [_ptr(v) for v in keep], 0, int(device), keep, None


def _seg_u32(torch, n, like):
    """An index array of capacity n where the cloud lives; (array, pointer)."""
    if torch is not None:
        a = torch.zeros(max(n, 1), dtype=torch.int32, device=like.device)
        return a, _dptr(a)
    a = np.zeros(max(n, 1), dtype=np.uint32)
    return a, _ptr(a)


def _seg_take(torch, a, k):
    return (a[:k].long() & 0xFFFFFFFF) if torch is not None else a[:k].copy()


def segment_ground(x, y, z, grid_resolution=0.5, cell_percentile=0.2, ground_thickness=0.3, max_ground_height=0.5,
                   min_points_per_cell=2, device=0):
    """nanopcl::segmentation::segmentGround(cloud, config) on the device: (ground, obstacles), the point indices of each
    in ascending order — uint32 numpy arrays for numpy input, int64 device tensors for torch device tensors."""
    lib = capi.load()
    n, ptrs, on_device, dev, keep, torch = _seg_cloud(x, y, z, device)
    cfg = capi.FdmGroundSegConfig(float(np.float32(grid_resolution)), float(np.float32(cell_percentile)),
                                  float(np.float32(ground_thickness)), float(np.float32(max_ground_height)),
                                  int(min_points_per_cell))
    ground, pg = _seg_u32(torch, n, keep[0])
    obstacles, po = _seg_u32(torch, n, keep[0])
    ng, no = C.c_uint64(0), C.c_uint64(0)
    _ck(lib.fdm_cloud_segment_ground(n, *ptrs, on_device, C.byref(cfg), dev, pg, po, C.byref(ng), C.byref(no)))
    return _seg_take(torch, ground, int(ng.value)), _seg_take(torch, obstacles, int(no.value))


class RansacResult:
    """nanopcl::segmentation::RansacResult: coefficients (float32[4]: nx, ny, nz, d), inliers (indices into the cloud, in
    index-list order), fitness, iterations, success."""

    def __init__(self, coefficients, inliers, fitness, iterations, success):
        self.coefficients, self.inliers = coefficients, inliers
        self.fitness, self.iterations, self.success = float(fitness), int(iterations), bool(success)

    def outliers(self, total):
        """RansacResult::outliers(total_points): the indices 0 .. total - 1 that are no inlier, ascending."""
        if _is_torch(self.inliers):
            import torch
            mask = torch.ones(int(total), dtype=torch.bool, device=self.inliers.device)
            mask[self.inliers] = False
            return torch.nonzero(mask).reshape(-1)
        mask = np.ones(int(total), dtype=bool)
        mask[self.inliers] = False
        return np.nonzero(mask)[0].astype(np.uint32)

    def __repr__(self):
        return (f"RansacResult(success={self.success}, coefficients={self.coefficients.tolist()}, "
                f"inliers={len(self.inliers)}, fitness={self.fitness:.6f}, iterations={self.iterations})")


def _ransac_config(distance_threshold, max_iterations, probability, min_inliers, refine_model):
    return capi.FdmRansacConfig(float(np.float32(distance_threshold)), int(max_iterations), float(probability),
                                int(min_inliers), 1 if refine_model else 0)


def _ransac_result(torch, r, inliers):
    return RansacResult(np.array(r.coefficients, dtype=np.float32), _seg_take(torch, inliers, int(r.n_inliers)),
                        r.fitness, r.iterations, r.success)


def segment_plane(x, y, z, distance_threshold=0.1, max_iterations=1000, probability=0.99, min_inliers=3,
                  refine_model=True, indices=None, device=0):
    """nanopcl::segmentation::segmentPlane (RANSAC, fixed seed) over the whole cloud or over `indices` (positions are
    sampled in that list, which may repeat a point).  Returns a RansacResult; its inliers are a uint32 numpy array for
    numpy input, an int64 device tensor for torch device tensors."""
    lib = capi.load()
    n, ptrs, on_device, dev, keep, torch = _seg_cloud(x, y, z, device)
    cfg = _ransac_config(distance_threshold, max_iterations, probability, min_inliers, refine_model)
    p_idx, m, idx = None, n, None
    if indices is not None:
        if torch is not None:
            idx = indices.to(device=keep[0].device, dtype=torch.int64).to(torch.int32).contiguous()
            p_idx, m = _dptr(idx), idx.numel()
        else:
            idx = np.ascontiguousarray(np.asarray(indices).astype(np.uint32)).reshape(-1)
            p_idx, m = _ptr(idx), idx.size
    inliers, pi = _seg_u32(torch, m, keep[0])
    r = capi.FdmRansacResult()
    _ck(lib.fdm_cloud_segment_plane(n, *ptrs, on_device, p_idx, m, C.byref(cfg), dev, pi, C.byref(r)))
    del idx
    return _ransac_result(torch, r, inliers)


def segment_multiple_planes(x, y, z, distance_threshold=0.1, max_iterations=1000, probability=0.99, min_inliers=3,
                            refine_model=True, max_planes=5, min_fitness=0.1, device=0):
    """nanopcl::segmentation::segmentMultiplePlanes: planes are taken one after the other, each from the points the
    earlier ones left, until max_planes, fewer than 3 points, or a result without success or below min_fitness.
    Returns a list of RansacResult."""
    lib = capi.load()
    n, ptrs, on_device, dev, keep, torch = _seg_cloud(x, y, z, device)
    cfg = _ransac_config(distance_threshold, max_iterations, probability, min_inliers, refine_model)
    inliers, pi = _seg_u32(torch, n, keep[0])
    res = (capi.FdmRansacResult * max(int(max_planes), 1))()
    count = C.c_uint64(0)
    _ck(lib.fdm_cloud_segment_planes(n, *ptrs, on_device, C.byref(cfg), int(max_planes), float(min_fitness), dev, pi, res,
                                     C.byref(count)))
    out, at = [], 0
    for k in range(int(count.value)):
        out.append(_ransac_result(torch, res[k], inliers[at:]))
        at += int(res[k].n_inliers)
    return out


def segment_last_stats():
    """What this thread's last segmentation call did: n_batches (launches of the scoring kernel), n_hypotheses,
    n_invalid_samples, batch (iterations per launch), ms (zeros unless fdm_cloud_debug_profile is on)."""
    st = capi.FdmSegmentStats()
    _ck(capi.load().fdm_segment_last_stats(C.byref(st)))
    return {"n_batches": int(st.n_batches), "n_hypotheses": int(st.n_hypotheses),
            "n_invalid_samples": int(st.n_invalid_samples), "batch": int(st.batch), "ms": tuple(float(v) for v in st.ms)}


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
        if _is_torch(self.indices):
            import torch
            mask = torch.ones(int(total), dtype=torch.bool, device=self.indices.device)
            mask[self.indices] = False
            return torch.nonzero(mask).reshape(-1)
        mask = np.ones(int(total), dtype=bool)
        mask[self.indices] = False
        return np.nonzero(mask)[0].astype(np.uint32)

    def __repr__(self):
        return f"ClusterResult(num_clusters={self.num_clusters}, total_clustered_points={self.total_clustered_points})"


def euclidean_cluster(x, y, z, indices=None, tolerance=0.5, min_size=10, max_size=100000, device=0):
    """nanopcl::segmentation::euclideanCluster on the device over the whole cloud or over `indices` (the values written
    are then the list's entries, i.e. indices into the cloud; a duplicate entry counts as two points).  Returns a
    ClusterResult; the relation and the order are stated in include/fdm_engine.h."""
    lib = capi.load()
    n, ptrs, on_device, dev, keep, torch = _seg_cloud(x, y, z, device)
    cfg = capi.FdmClusterConfig(float(np.float32(tolerance)), int(min_size), int(max_size))
    p_idx, m, idx = None, n, None
    if indices is not None:
        if torch is not None:
            idx = indices.to(device=keep[0].device, dtype=torch.int64).to(torch.int32).contiguous()
            p_idx, m = _dptr(idx), idx.numel()
        else:
            idx = np.ascontiguousarray(np.asarray(indices).astype(np.uint32)).reshape(-1)
            p_idx, m = _ptr(idx), idx.size
    out, po = _seg_u32(torch, m, keep[0])
    offsets, pf = _seg_u32(torch, m + 1, keep[0])
    labels, pl = _seg_u32(torch, m, keep[0])
    count = C.c_uint64(0)
    _ck(lib.fdm_cloud_cluster(n, *ptrs, on_device, p_idx, m, C.byref(cfg), dev, po, pf, pl, C.byref(count)))
    del idx
    k = int(count.value)
    off = _seg_take(torch, offsets, k + 1)
    return ClusterResult(_seg_take(torch, out, int(off[k])), off, _seg_take(torch, labels, m))


def apply_cluster_labels(result, total, semantic_class=0):
    """nanopcl::segmentation::applyClusterLabels: the uint32 Label channel of a cloud of `total` points,
    (semantic_class << 16) | uint16(cluster number + 1) for a clustered point — the instance id truncated to 16 bits as
    in the reference — and (semantic_class << 16) for noise.  A numpy array."""
    sem = np.uint32((int(semantic_class) & 0xFFFF) << 16)
    out = np.full(int(total), sem, dtype=np.uint32)
    ind = result.indices.cpu().numpy() if _is_torch(result.indices) else np.asarray(result.indices)
    off = result.offsets.cpu().numpy() if _is_torch(result.offsets) else np.asarray(result.offsets)
    if ind.size:
        sizes = np.diff(off.astype(np.int64))
        ids = (np.arange(sizes.size, dtype=np.int64) + 1) & 0xFFFF
        out[ind.astype(np.int64)] = sem | np.repeat(ids, sizes).astype(np.uint32)
    return out


def cluster_last_stats():
    """What this thread's last euclidean_cluster did: the counts of fdm_cluster_stats and ms (zeros unless
    fdm_cloud_debug_profile is on)."""
    st = capi.FdmClusterStats()
    _ck(capi.load().fdm_cluster_last_stats(C.byref(st)))
    out = {k: int(getattr(st, k)) for k, _ in capi.FdmClusterStats._fields_ if k != "ms"}
    out["ms"] = tuple(float(v) for v in st.ms)
    return out
