// fdm_engine_raster.inl — host side of fromPointCloud / toPointCloud (fdm_raster.hpp; reference: pcd_convert.cpp).
// Part of fdm_engine_post.hip (one of the library's five translation units, fdm_engine_host.hpp).
// Every entry is synchronous: whether any layer is created at all depends on a count only the device knows.

namespace {
constexpr uint64_t kRasMaxPoints = 1ull << 31;

bool whole_map(const fdm_engine* e) { return e->G.s_rows == e->G.rows && e->G.s_cols == e->G.cols; }

// keys / indices of the sort (both sides of its ping-pong) and its histograms, for n points; the shared counters
int ensure_raster_scratch(fdm_engine* e, size_t n) {
  if (!e->pc_stat) HIPCK(hipMalloc(reinterpret_cast<void**>(&e->pc_stat), sizeof(RasterStat)));
  if (n <= e->pc_cap) return FDM_OK;
  if (int rc_sync = sync_all(e)) return rc_sync;
  for (int k = 0; k < 2; ++k) {
    if (e->pc_keys[k]) HIPCK(hipFree(e->pc_keys[k]));
    if (e->pc_idx[k]) HIPCK(hipFree(e->pc_idx[k]));
    e->pc_keys[k] = e->pc_idx[k] = nullptr;
  }
  if (e->pc_hist) HIPCK(hipFree(e->pc_hist));
  e->pc_hist = nullptr;
  e->pc_cap = 0;
  const size_t cap = n + n / 4 + 1024;
  for (int k = 0; k < 2; ++k) {
    HIPCK(hipMalloc(reinterpret_cast<void**>(&e->pc_keys[k]), cap * sizeof(uint32_t)));
    HIPCK(hipMalloc(reinterpret_cast<void**>(&e->pc_idx[k]), cap * sizeof(uint32_t)));
  }
  // 256 bins x tiles + the 256 totals (fdm_rsort.hpp), for either tile size
  const size_t tiles = std::max((cap + kRsTile - 1) / kRsTile, (size_t(kRsSmallMax) + kRsTileSmall - 1) / kRsTileSmall);
  HIPCK(hipMalloc(reinterpret_cast<void**>(&e->pc_hist), (256u * tiles + 256u) * sizeof(uint32_t)));
  e->pc_cap = cap;
  return FDM_OK;
}

// stable sort of (pc_keys[0], position) by the low `bits` bits; returns the side the result is on
template <unsigned TILE>
int raster_sort_t(fdm_engine* e, unsigned n, unsigned bits) {
  const unsigned tiles = (n + TILE - 1u) / TILE;
  uint32_t* const hist = e->pc_hist;
  uint32_t* const total = hist + size_t(256) * tiles;
  int src = 0;
  for (unsigned shift = 0; shift < bits; shift += 8u, src ^= 1) {
    hipLaunchKernelGGL((k_rs_hist<uint32_t, TILE>), dim3(tiles), dim3(256), 0, e->stream, n, e->pc_keys[src], shift,
                       tiles, hist);
    hipLaunchKernelGGL(k_rs_scan, dim3(256), dim3(256), 0, e->stream, tiles, hist, total);
    if (shift)
      hipLaunchKernelGGL((k_rs_scatter<uint32_t, true, int(TILE / 256u)>), dim3(tiles), dim3(256), 0, e->stream, n,
                         e->pc_keys[src], e->pc_idx[src], e->pc_keys[src ^ 1], e->pc_idx[src ^ 1], shift, tiles, hist,
                         total);
    else
      hipLaunchKernelGGL((k_rs_scatter<uint32_t, false, int(TILE / 256u)>), dim3(tiles), dim3(256), 0, e->stream, n,
                         e->pc_keys[src], static_cast<const uint32_t*>(nullptr), e->pc_keys[src ^ 1],
                         e->pc_idx[src ^ 1], shift, tiles, hist, total);
  }
  return src;
}

// `map.add(name, value)` of a layer the map does not show yet (pcd_convert.cpp:106-112): a new layer, or a lazily
// allocated one that no scan has made visible — which the reference does not have, so it is born now, at the end
int raster_ensure_layer(fdm_engine* e, const char* name, float value) {
  Layer* l = find_layer(e, name);
  if (!l) return add_layer(e, name, value, false);
  if (!l->pending) return FDM_OK;
  Layer born = *l;
  born.pending = false;
  e->layers.erase(e->layers.begin() + (l - e->layers.data()));
  e->layers.push_back(born);
  return fill_async(e, lptr(e, born), value, e->ncell, lstride(e, born));
}

int read_raster_stat(fdm_engine* e, RasterStat* h) {
  HIPCK(hipMemcpyAsync(h, e->pc_stat, sizeof(RasterStat), hipMemcpyDeviceToHost, e->stream));
  return sync_all(e);
}

// option fdm_engine_enable_profile: device time of the call's three phases (fdm_engine_last_raster_ms), on events of
// the path's own (pc_ev: the scan path's ev[] keep what fdm_engine_last_kernel_ms reports): [0] [1] around the id kernel,
// [2] [3] [4] before the sort, between sort and walk, behind the walk
int ensure_raster_events(fdm_engine* e) {
  if (!e->profile) return FDM_OK;
  for (auto& ev : e->pc_ev)
    if (!ev) HIPCK(hipEventCreate(&ev));
  return FDM_OK;
}
void mark(fdm_engine* e, int k) {
  if (e->profile) (void)hipEventRecord(e->pc_ev[k], e->stream);
}

// fromPointCloud(cloud, map, method) on device arrays; the engine's stream is joined, arguments are checked
int raster_device(fdm_engine* e, uint64_t n, const float* dx, const float* dy, const float* dz, const float* dint,
                  const uint32_t* drgb, int method, fdm_raster_stats* out) {
  int rc;
  if ((rc = resolve_pending(e))) return rc;
  if ((rc = ensure_raster_scratch(e, size_t(n)))) return rc;
  if ((rc = ensure_raster_events(e))) return rc;
  const unsigned np = unsigned(n), blocks = (np + 255u) / 256u;
  const int slot = int(e->scan_no & 3);
  const uint32_t ncell = uint32_t(e->ncell);
  mark(e, 0);
  hipLaunchKernelGGL(k_ras_stat_init, dim3(1), dim3(64), 0, e->stream, e->pc_stat);
  hipLaunchKernelGGL(k_ras_ids, dim3(blocks), dim3(256), 0, e->stream, np, dx, dy, dz, e->G, e->d_state, slot, ncell,
                     e->pc_keys[0], e->pc_stat);
  HIPCK(hipGetLastError());
  mark(e, 1);
  RasterStat hs{};
  if ((rc = read_raster_stat(e, &hs))) return rc;
  if (out) out->n_points_used = hs.n_used;
  e->pc_ms[0] = e->pc_ms[1] = e->pc_ms[2] = 0.f;
  if (e->profile) (void)hipEventElapsedTime(&e->pc_ms[0], e->pc_ev[0], e->pc_ev[1]);
  if (hs.n_used == 0u) return FDM_SKIP_NO_CELL;  // pcd_convert.cpp:103
  if (!find_layer(e, "elevation")) return fail(FDM_ERR_NO_LAYER, "no layer elevation");
  if ((rc = raster_ensure_layer(e, "elevation_min", NAN))) return rc;
  if ((rc = raster_ensure_layer(e, "elevation_max", NAN))) return rc;
  if ((rc = raster_ensure_layer(e, "variance", NAN))) return rc;
  if ((rc = raster_ensure_layer(e, "n_points", 0.0f))) return rc;
  if (dint && (rc = raster_ensure_layer(e, "intensity", NAN))) return rc;
  if (drgb && (rc = raster_ensure_layer(e, "color", NAN))) return rc;
  static const char* const kNames[kRasLayers] = {"elevation", "elevation_min", "elevation_max", "variance",
                                                 "n_points", "intensity", "color"};
  RasterLayers RL{};
  for (int k = 0; k < kRasLayers; ++k) {
    RL.p[k] = nullptr;
    RL.s[k] = 1;
    if ((k == kRasIntensity && !dint) || (k == kRasColor && !drgb)) continue;
    RL.p[k] = Lany(e, kNames[k], &RL.s[k]);
  }
  unsigned bits = 1;
  while (bits < 32u && (uint64_t(ncell) >> bits) != 0u) ++bits;  // the keys are 0 .. ncell
  mark(e, 2);
  const int side = rs_tile(np) == kRsTileSmall ? raster_sort_t<kRsTileSmall>(e, np, bits)
                                               : raster_sort_t<kRsTile>(e, np, bits);
  HIPCK(hipGetLastError());
  mark(e, 3);
  hipLaunchKernelGGL(k_ras_walk, dim3(blocks), dim3(256), 0, e->stream, np, e->pc_keys[side], e->pc_idx[side], ncell,
                     dz, dint, drgb, method, RL, e->pc_stat);
  HIPCK(hipGetLastError());
  mark(e, 4);
  if ((rc = read_raster_stat(e, &hs))) return rc;
  if (out) out->n_cells_written = hs.n_cells;
  if (e->profile) {
    (void)hipEventElapsedTime(&e->pc_ms[1], e->pc_ev[2], e->pc_ev[3]);
    (void)hipEventElapsedTime(&e->pc_ms[2], e->pc_ev[3], e->pc_ev[4]);
  }
  return FDM_OK;
}

int check_raster_args(fdm_engine* e, uint64_t n, const float* x, const float* y, const float* z, int method,
                      fdm_raster_stats* out) {
  if (out) out->n_points_used = out->n_cells_written = 0;
  if (!e) return fail(FDM_ERR_INVALID, "null engine");
  if (!whole_map(e)) return fail(FDM_ERR_INVALID, "fromPointCloud is not defined for tiled engines");
  if (n >= kRasMaxPoints) return fail(FDM_ERR_INVALID, "point count exceeds 2^31-1");
  if (method < 0 || method > 3) return fail(FDM_ERR_INVALID, "method must be 0 (Max), 1 (Min), 2 (Mean) or 3 (MinMax)");
  if (n && (!x || !y || !z)) return fail(FDM_ERR_INVALID, "null coordinate array");
  return FDM_OK;
}

// five channels of `cap` points each in ONE allocation: x | y | z | intensity | rgb
int grow_channels(fdm_engine* e, float** buf, size_t* cap, size_t n) {
  if (n <= *cap) return FDM_OK;
  if (int rc_sync = sync_all(e)) return rc_sync;
  if (*buf) HIPCK(hipFree(*buf));
  *buf = nullptr;
  *cap = 0;
  const size_t c = ((n + n / 4 + 1024) + 3) & ~size_t(3);
  HIPCK(hipMalloc(reinterpret_cast<void**>(buf), c * 5 * sizeof(float)));
  *cap = c;
  return FDM_OK;
}
}  // namespace

extern "C" {

int fdm_engine_from_point_cloud_device(fdm_engine* e, uint64_t n, const float* dx, const float* dy, const float* dz,
                                       const float* dintensity, const uint32_t* drgb, int method,
                                       fdm_raster_stats* out) {
  if (int rc = join_streams(e)) return rc;  // a held-back update is applied before the first write
  if (int rc = check_raster_args(e, n, dx, dy, dz, method, out)) return rc;
  if (n == 0) return FDM_SKIP_EMPTY_CLOUD;  // pcd_convert.cpp:65
  HIPCK(hipSetDevice(e->device));
  return raster_device(e, n, dx, dy, dz, dintensity, drgb, method, out);
}

int fdm_engine_from_point_cloud(fdm_engine* e, uint64_t n, const float* x, const float* y, const float* z,
                                const float* intensity, const uint32_t* rgb, int method, fdm_raster_stats* out) {
  if (int rc = join_streams(e)) return rc;
  if (int rc = check_raster_args(e, n, x, y, z, method, out)) return rc;
  if (n == 0) return FDM_SKIP_EMPTY_CLOUD;
  HIPCK(hipSetDevice(e->device));
  if (int rc = grow_channels(e, &e->pc_in, &e->pc_in_cap, size_t(n))) return rc;
  const size_t cap = e->pc_in_cap, bytes = size_t(n) * sizeof(float);
  float* const d = e->pc_in;
  const void* const src[5] = {x, y, z, intensity, rgb};
  for (int k = 0; k < 5; ++k)
    if (src[k]) HIPCK(hipMemcpyAsync(d + cap * size_t(k), src[k], bytes, hipMemcpyHostToDevice, e->stream));
  return raster_device(e, n, d, d + cap, d + 2 * cap, intensity ? d + 3 * cap : nullptr,
                       rgb ? reinterpret_cast<const uint32_t*>(d + 4 * cap) : nullptr, method, out);
}

// fromPointCloud(cloud, resolution, method): pcd_convert.cpp:155-185
int fdm_engine_create_from_point_cloud(uint64_t n, const void* x, const void* y, const void* z, const void* intensity,
                                       const void* rgb, int on_device, float resolution, int method, int device,
                                       fdm_engine** out_engine, fdm_raster_stats* out) {
  if (out) out->n_points_used = out->n_cells_written = 0;
  if (!out_engine) return fail(FDM_ERR_INVALID, "null argument");
  *out_engine = nullptr;
  if (n == 0) return FDM_SKIP_EMPTY_CLOUD;  // `return {}`: no map
  if (n >= kRasMaxPoints) return fail(FDM_ERR_INVALID, "point count exceeds 2^31-1");
  if (method < 0 || method > 3) return fail(FDM_ERR_INVALID, "method must be 0 (Max), 1 (Min), 2 (Mean) or 3 (MinMax)");
  if (!x || !y || !z) return fail(FDM_ERR_INVALID, "null coordinate array");
  if (!(resolution > 0.0f) || !std::isfinite(resolution)) return fail(FDM_ERR_INVALID, "resolution must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(FDM_ERR_NO_DEVICE, "no HIP device: the engine has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(FDM_ERR_INVALID, "bad device ordinal");
  HIPCK(hipSetDevice(device));
  // the cloud on the device (host arrays: one staging block for the whole call), then its bounding box
  const void* src[5] = {x, y, z, intensity, rgb};
  const float* ch[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  float* stage = nullptr;
  RasterStat* d_stat = nullptr;
  fdm_engine* e = nullptr;
  auto done = [&](int rc) {
    if (stage) (void)hipFree(stage);
    if (d_stat) (void)hipFree(d_stat);
    if (rc < 0 && e) { fdm_engine_destroy(e); e = nullptr; }
    *out_engine = e;
    return rc;
  };
#define RCK(expr)                                                                                           \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess) return done(fail(FDM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e))); \
  } while (0)
  if (on_device) {
    for (int k = 0; k < 5; ++k) ch[k] = static_cast<const float*>(src[k]);
  } else {
    const size_t cap = (size_t(n) + 3) & ~size_t(3);
    RCK(hipMalloc(reinterpret_cast<void**>(&stage), cap * 5 * sizeof(float)));
    for (int k = 0; k < 5; ++k) {
      if (!src[k]) continue;
      RCK(hipMemcpy(stage + cap * size_t(k), src[k], size_t(n) * sizeof(float), hipMemcpyHostToDevice));
      ch[k] = stage + cap * size_t(k);
    }
  }
  RCK(hipMalloc(reinterpret_cast<void**>(&d_stat), sizeof(RasterStat)));
  const unsigned np = unsigned(n);
  hipLaunchKernelGGL(k_ras_stat_init, dim3(1), dim3(64), 0, nullptr, d_stat);
  hipLaunchKernelGGL(k_ras_bounds, dim3(std::min((np + 255u) / 256u, 2048u)), dim3(256), 0, nullptr, np, ch[0], ch[1],
                     d_stat);
  RCK(hipGetLastError());
  RasterStat hs{};
  RCK(hipMemcpy(&hs, d_stat, sizeof(hs), hipMemcpyDeviceToHost));
  auto unord_host = [](uint32_t u) {
    const uint32_t b = u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    float f;
    std::memcpy(&f, &b, sizeof(f));
    return f;
  };
  const float min_x = unord_host(hs.min_x), min_y = unord_host(hs.min_y);
  const float max_x = unord_host(hs.max_x), max_y = unord_host(hs.max_y);
  // one cell of margin (:175-176), in fp32 as the reference computes it
  const float width = max_x - min_x + resolution, height = max_y - min_y + resolution;
  // an extent that is not a positive finite number (no point with both coordinates, an infinite coordinate) is
  // undefined behaviour in the reference (a map of no or of 2^31 cells): refused here
  if (!std::isfinite(width) || !std::isfinite(height) || !(width > 0.0f) || !(height > 0.0f))
    return done(fail(FDM_ERR_INVALID, "the cloud's x / y extent is not a positive finite number"));
  fdm_geometry g{};
  g.length_x = double(width);       // ElevationMap::setGeometry(float, float, float): promoted
  g.length_y = double(height);
  g.resolution = double(resolution);
  g.position_x = double(min_x + max_x) / 2.0;  // an fp32 sum, an fp64 divide (:180-181)
  g.position_y = double(min_y + max_y) / 2.0;
  int rc = fdm_engine_create_map(&g, nullptr, device, &e);
  if (rc) { e = nullptr; return done(rc); }
  rc = fdm_engine_from_point_cloud_device(e, n, ch[0], ch[1], ch[2], ch[3],
                                          reinterpret_cast<const uint32_t*>(ch[4]), method, out);
  return done(rc < 0 ? rc : FDM_OK);  // (a cloud that reaches no cell still has its map, with the three basic layers)
#undef RCK
}

// toPointCloud(map) -> SoA channels in an engine-owned buffer (valid until the next call of either variant)
int fdm_engine_to_point_cloud_device(fdm_engine* e, const float** dx, const float** dy, const float** dz,
                                     const float** dintensity, const uint32_t** drgb, uint64_t* n_points,
                                     int32_t* has_intensity, int32_t* has_color) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !n_points) return fail(FDM_ERR_INVALID, "null argument");
  if (!whole_map(e)) return fail(FDM_ERR_INVALID, "toPointCloud is not defined for tiled engines");
  HIPCK(hipSetDevice(e->device));
  int rc;
  if ((rc = resolve_pending(e))) return rc;
  Layer* elev = find_layer(e, "elevation");
  if (!elev || elev->pending) return fail(FDM_ERR_NO_LAYER, "no layer elevation");
  CloudLayers CL{};
  CL.elev = lptr(e, *elev);
  CL.elev_stride = lstride(e, *elev);
  CL.int_stride = 1;
  if (Layer* l = find_layer(e, "intensity"); l && !l->pending) { CL.intensity = lptr(e, *l); CL.int_stride = lstride(e, *l); }
  if (Layer* l = find_layer(e, "color"); l && !l->pending) CL.color = lptr(e, *l);
  if ((rc = ensure_raster_scratch(e, 0))) return rc;
  const unsigned long long total = (unsigned long long)e->G.rows * e->G.cols;
  const unsigned blocks = unsigned((total + 255) / 256);
  if (size_t(blocks) + 1 > e->pack_counts_cap) {
    if (int rc_sync = sync_all(e)) return rc_sync;
    if (e->pack_counts) HIPCK(hipFree(e->pack_counts));
    e->pack_counts_cap = size_t(blocks) + 1 + 1024;
    HIPCK(hipMalloc(reinterpret_cast<void**>(&e->pack_counts), e->pack_counts_cap * sizeof(uint32_t)));
  }
  const int slot = int(e->scan_no & 3);
  hipLaunchKernelGGL(k_ras_stat_init, dim3(1), dim3(64), 0, e->stream, e->pc_stat);
  hipLaunchKernelGGL(k_cloud_count, dim3(blocks), dim3(256), 0, e->stream, e->G, e->d_state, slot, CL, e->pack_counts,
                     e->pc_stat);
  hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, e->stream, e->pack_counts, blocks);
  HIPCK(hipGetLastError());
  uint32_t count = 0;
  HIPCK(hipMemcpyAsync(&count, e->pack_counts + blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  RasterStat hs{};
  if ((rc = read_raster_stat(e, &hs))) return rc;
  if ((rc = grow_channels(e, &e->pc_out, &e->pc_out_cap, std::max<size_t>(count, 1)))) return rc;
  if (count) {
    hipLaunchKernelGGL(k_cloud_write, dim3(blocks), dim3(256), 0, e->stream, e->G, e->d_state, slot, CL,
                       e->pack_counts, e->pc_out, e->pc_out_cap);
    HIPCK(hipGetLastError());
    if ((rc = sync_all(e))) return rc;
  }
  const size_t cap = e->pc_out_cap;
  *n_points = count;
  if (dx) *dx = e->pc_out;
  if (dy) *dy = e->pc_out + cap;
  if (dz) *dz = e->pc_out + 2 * cap;
  if (dintensity) *dintensity = e->pc_out + 3 * cap;
  if (drgb) *drgb = reinterpret_cast<const uint32_t*>(e->pc_out + 4 * cap);
  if (has_intensity) *has_intensity = hs.has_int ? 1 : 0;
  if (has_color) *has_color = hs.has_col ? 1 : 0;
  return FDM_OK;
}

// ... and copied to the host: arrays of `cap` points each (any may be NULL).  *n_points is always the cloud's size; a
// cloud larger than `cap` is not copied and the status says so (FDM_SKIP_BUFFER_TOO_SMALL: call again with room for
// *n_points, or with rows * cols in the first place).
int fdm_engine_to_point_cloud(fdm_engine* e, uint64_t cap, float* x, float* y, float* z, float* intensity,
                              uint32_t* rgb, uint64_t* n_points, int32_t* has_intensity, int32_t* has_color) {
  const float *dx = nullptr, *dy = nullptr, *dz = nullptr, *di = nullptr;
  const uint32_t* dc = nullptr;
  if (int rc = fdm_engine_to_point_cloud_device(e, &dx, &dy, &dz, &di, &dc, n_points, has_intensity, has_color))
    return rc;
  const uint64_t n = *n_points;
  if (n == 0) return FDM_OK;
  if (n > cap) return FDM_SKIP_BUFFER_TOO_SMALL;
  void* const dst[5] = {x, y, z, intensity, rgb};
  const void* const src[5] = {dx, dy, dz, di, dc};
  for (int k = 0; k < 5; ++k)
    if (dst[k]) HIPCK(hipMemcpyAsync(dst[k], src[k], size_t(n) * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  return sync_all(e);
}

// ms3: device time of the last fromPointCloud's cell ids, grouping (the sort) and walk; zeros unless
// fdm_engine_enable_profile was on
int fdm_engine_last_raster_ms(fdm_engine* e, float* ms3) {
  if (!e || !ms3) return fail(FDM_ERR_INVALID, "null argument");
  for (int k = 0; k < 3; ++k) ms3[k] = e->pc_ms[k];
  return FDM_OK;
}

}  // extern "C"
