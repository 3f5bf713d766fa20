// fdm_engine_raster.inl — host side of fromPointCloud / toPointCloud (fdm_raster.hpp; reference: pcd_convert.cpp).
// Part of fdm_engine_post.hip (one of the library's five translation units, fdm_engine_host.hpp), behind
// fdm_engine_cloud.inl, whose helpers it uses.
// Every entry is synchronous: whether any layer is created at all depends on a count only the device knows.

namespace {
bool whole_map(const fdm_engine* e) { return e->G.s_rows == e->G.rows && e->G.s_cols == e->G.cols; }

// keys / indices of the sort (both sides of its ping-pong) and its histograms, for n points; the shared counters
int ensure_raster_scratch(fdm_engine* e, size_t n) {
  if (!e->pc_stat) HIPCK(hipMalloc(reinterpret_cast<void**>(&e->pc_stat), sizeof(RasterStat)));
  if (n <= e->pc_cap) return FDM_OK;
  // five buffers under ONE capacity, pc_cap, which is 0 until all five are there.  Each is replaced through grow_device
  // with a capacity of its own that says "empty" (the first call drains the engine, the others find it idle), in the
  // order they have always been allocated in: keys, indices, keys, indices, histogram
  const size_t want = n + n / 4 + 1024;
  e->pc_cap = 0;
  for (uint32_t** p : {&e->pc_keys[0], &e->pc_idx[0], &e->pc_keys[1], &e->pc_idx[1]}) {
    size_t none = 0;
    if (int rc = grow_device(e, p, &none, want, want)) return rc;
  }
  size_t none = 0;
  const size_t words = rs_hist_words(want);
  if (int rc = grow_device(e, &e->pc_hist, &none, words, words)) return rc;
  e->pc_cap = want;
  return FDM_OK;
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
  mark(e, 2);
  const RsPairs<uint32_t> pairs{{e->pc_keys[0], e->pc_keys[1]}, {e->pc_idx[0], e->pc_idx[1]}, e->pc_hist};
  const int side = rs_enqueue(e->stream, pairs, np, rs_key_bits(ncell));  // the keys are 0 .. ncell
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
  return check_cloud(n, x, y, z, method);
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
  if (int rc = grow_device(e, &e->pc_in, &e->pc_in_cap, size_t(n), cloud_cap(size_t(n)), 5)) return rc;
  const void* const src[5] = {x, y, z, intensity, rgb};
  const float* ch[5];
  if (int rc = upload_cloud(e->stream, n, 5, src, e->pc_in, e->pc_in_cap, ch)) return rc;
  return raster_device(e, n, ch[0], ch[1], ch[2], ch[3], reinterpret_cast<const uint32_t*>(ch[4]), method, out);
}

// fromPointCloud(cloud, resolution, method): pcd_convert.cpp:155-185
int fdm_engine_create_from_point_cloud(uint64_t n, const void* x, const void* y, const void* z, const void* intensity,
                                       const void* rgb, int on_device, float resolution, int method, int device,
                                       fdm_engine** out_engine, fdm_raster_stats* out) {
  if (out) out->n_points_used = out->n_cells_written = 0;
  if (!out_engine) return fail(FDM_ERR_INVALID, "null argument");
  *out_engine = nullptr;
  if (n == 0) return FDM_SKIP_EMPTY_CLOUD;  // `return {}`: no map
  if (int rc = check_cloud(n, x, y, z, method)) return rc;
  if (int rc = check_resolution(resolution)) return rc;
  if (int rc = pick_device(device)) return rc;
  // the cloud on the device (host arrays: one staging block for the whole call), then the map over its bounding box
  const void* const src[5] = {x, y, z, intensity, rgb};
  const float* ch[5];
  CloudBlock stage;
  if (int rc = stage_cloud(nullptr, n, 5, src, on_device != 0, stage, ch)) return rc;
  fdm_engine* e = nullptr;
  if (int rc = map_over_cloud(unsigned(n), ch[0], ch[1], resolution, device, &e)) return rc;
  const int rc = fdm_engine_from_point_cloud_device(e, n, ch[0], ch[1], ch[2], ch[3],
                                                    reinterpret_cast<const uint32_t*>(ch[4]), method, out);
  if (rc < 0) {
    fdm_engine_destroy(e);
    return rc;
  }
  *out_engine = e;  // (a cloud that reaches no cell still has its map, with the three basic layers)
  return FDM_OK;
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
  if ((rc = ensure_pack_counts(e, blocks))) return rc;
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
  const size_t n_out = std::max<size_t>(count, 1);
  if ((rc = grow_device(e, &e->pc_out, &e->pc_out_cap, n_out, cloud_cap(n_out), 5))) return rc;
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
