// fdm_engine_opts.inl — scan-callback captures, per-point cell ids, the per-launch profile and fdm_engine_set_option (the option table).
// Part of fdm_engine.hip's translation unit (inside its extern "C" block): do not compile on its own.

int fdm_engine_capture(fdm_engine* e, int preprocessed, int rasterized) {
  if (int rc = join_streams(e)) return rc;
  if (!e) return fail(FDM_ERR_INVALID, "null engine");
  e->cap_pre = preprocessed != 0;
  e->cap_cov = preprocessed == 2;
  e->cap_ras = rasterized != 0;
  if (e->cap_pre) e->want_ids = true;  // the per-point pass flag rides on the cell-id buffer
  return FDM_OK;
}

int fdm_engine_last_preprocessed(fdm_engine* e, uint64_t cap, float* x, float* y, float* z,
                                 float* sigma_z2, uint64_t* n_out) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !n_out) return fail(FDM_ERR_INVALID, "null argument");
  *n_out = 0;
  if (!e->cap_pre) return fail(FDM_ERR_INVALID, "preprocessed-scan capture is off");
  const size_t n = e->last_n;
  if (!e->have_scan || n == 0 || !e->d_cap || !e->d_cell_ids) return FDM_OK;
  if (int rc_sync = sync_all(e)) return rc_sync;
  std::vector<float> h(4 * n);
  std::vector<int32_t> ids(n);
  for (int c = 0; c < 4; ++c)
    HIPCK(hipMemcpy(h.data() + c * n, e->d_cap + c * e->cap_cap, n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(ids.data(), e->d_cell_ids, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  uint64_t w = 0;
  for (size_t i = 0; i < n; ++i) {  // order-preserving compaction = marshalling, like filterInPlace
    if (ids[i] == -1) continue;     // dropped by cropRange / cropZ
    if (w < cap) {
      if (x) x[w] = h[i];
      if (y) y[w] = h[n + i];
      if (z) z[w] = h[2 * n + i];
      if (sigma_z2) sigma_z2[w] = h[3 * n + i];
    }
    ++w;
  }
  *n_out = w;
  return FDM_OK;
}

int fdm_engine_last_preprocessed_cov(fdm_engine* e, uint64_t cap, float* cov9, uint64_t* n_out) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !n_out || !cov9) return fail(FDM_ERR_INVALID, "null argument");
  *n_out = 0;
  if (!e->cap_pre || !e->cap_cov) return fail(FDM_ERR_INVALID, "covariance capture is off (fdm_engine_capture(e, 2, ..))");
  const size_t n = e->last_n;
  if (!e->have_scan || n == 0 || !e->d_cap || !e->d_cell_ids) return FDM_OK;
  if (int rc_sync = sync_all(e)) return rc_sync;
  std::vector<float> h(9 * n);
  std::vector<int32_t> ids(n);
  for (int c = 0; c < 9; ++c)
    HIPCK(hipMemcpy(h.data() + c * n, e->d_cap + (4 + c) * e->cap_cap, n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(ids.data(), e->d_cell_ids, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  uint64_t w = 0;
  for (size_t i = 0; i < n; ++i) {  // the same order-preserving compaction as fdm_engine_last_preprocessed
    if (ids[i] == -1) continue;
    if (w < cap)
      for (int c = 0; c < 9; ++c) cov9[w * 9 + c] = h[c * n + i];
    ++w;
  }
  *n_out = w;
  return FDM_OK;
}

int fdm_engine_last_rasterized(fdm_engine* e, uint64_t cap, float* x, float* y, float* z,
                               uint64_t* n_out) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !n_out) return fail(FDM_ERR_INVALID, "null argument");
  *n_out = 0;
  if (!e->cap_ras) return fail(FDM_ERR_INVALID, "rasterized-scan capture is off");
  if (!e->have_scan || !e->d_ras) return FDM_OK;
  if (int rc_sync = sync_all(e)) return rc_sync;
  std::vector<float> h(e->ncell);
  HIPCK(hipMemcpy(h.data(), e->d_ras, e->ncell * sizeof(float), hipMemcpyDeviceToHost));
  fdm_geometry g;
  if (int rc = fdm_engine_get_geometry(e, &g)) return rc;
  uint64_t w = 0;
  const GeomConst& G = e->G;
  for (size_t o = 0; o < e->ncell; ++o) {
    if (std::isnan(h[o])) continue;
    if (w < cap) {
      const int r = int(o % size_t(G.s_rows)) + G.s_r0, c = int(o / size_t(G.s_rows)) + G.s_c0;
      int ur = r - g.start_row, uc = c - g.start_col;  // getPositionFromIndex (grid_map_core)
      if (ur < 0) ur += G.rows;
      if (uc < 0) uc += G.cols;
      const double px = g.position_x + (0.5 * G.len_x - 0.5 * G.res) + G.res * double(-ur);
      const double py = g.position_y + (0.5 * G.len_y - 0.5 * G.res) + G.res * double(-uc);
      if (x) x[w] = float(px);
      if (y) y[w] = float(py);
      if (z) z[w] = h[o];
    }
    ++w;
  }
  *n_out = w;
  return FDM_OK;
}

int fdm_engine_enable_cell_ids(fdm_engine* e, int on) {
  if (int rc = join_streams(e)) return rc;
  if (!e) return fail(FDM_ERR_INVALID, "null engine");
  e->want_ids = on != 0;
  return FDM_OK;
}

int fdm_engine_last_cell_ids(fdm_engine* e, int32_t* host_out, uint64_t n) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !host_out) return fail(FDM_ERR_INVALID, "null argument");
  if (!e->want_ids || !e->d_cell_ids || n != e->last_n)
    return fail(FDM_ERR_INVALID, "cell ids not recorded for the last scan");
  HIPCK(hipMemcpyAsync(host_out, e->d_cell_ids, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  if (int rc_sync = sync_all(e)) return rc_sync;
  return FDM_OK;
}

int fdm_engine_enable_profile(fdm_engine* e, int on) {
  if (int rc = join_streams(e)) return rc;
  if (!e) return fail(FDM_ERR_INVALID, "null engine");
  e->profile = on != 0;
  return FDM_OK;
}

int fdm_engine_last_kernel_ms(fdm_engine* e, float* ms2) {
  if (!e || !ms2) return fail(FDM_ERR_INVALID, "null argument");
  if (!e->profile) return fail(FDM_ERR_INVALID, "profiling is off");
  HIPCK(hipEventSynchronize(e->ev[3]));  // no flush: a held-back update stays held (the chain is what is timed)
  // an event pair around ONE short kernel also times the gap to the next command; the empty
  // pair (ev2 -> ev3) measures that gap and is subtracted, so the figures agree with rocprofv3
  float raw0 = 0.f, raw1 = 0.f, gap = 0.f;
  HIPCK(hipEventElapsedTime(&raw0, e->ev[0], e->ev[1]));
  HIPCK(hipEventElapsedTime(&raw1, e->ev[1], e->ev[2]));
  HIPCK(hipEventElapsedTime(&gap, e->ev[2], e->ev[3]));
  ms2[0] = raw0 > gap ? raw0 - gap : raw0;
  ms2[1] = e->chain ? 0.0f : (raw1 > gap ? raw1 - gap : raw1);  // held back: it rides with the next launch
  return FDM_OK;
}

// ---- fdm_engine_set_option: one table (kOptions), one lookup-and-apply routine, four hooks ----
// What a row accepts and how the value is normalised before it is stored.
struct OptRule {
  enum Kind { kBool, kRaw, kAtLeast, kRange, kOneOf } kind;
  long long a, b;       // kAtLeast: clamp from below to a; kRange: a .. b inclusive; kOneOf: a = bit mask of the accepted values
  const char* accepts;  // the error message after "<name>: "
};
constexpr OptRule opt_bool() { return {OptRule::kBool, 0, 1, ""}; }  // stored as value != 0
constexpr OptRule opt_raw() { return {OptRule::kRaw, 0, 0, ""}; }    // measurement switches: any value
constexpr OptRule opt_at_least(long long lo) { return {OptRule::kAtLeast, lo, 0, ""}; }
constexpr OptRule opt_range(long long lo, long long hi, const char* accepts) { return {OptRule::kRange, lo, hi, accepts}; }
constexpr OptRule opt_one_of(unsigned long long mask, const char* accepts) {
  return {OptRule::kOneOf, static_cast<long long>(mask), 0, accepts};
}
constexpr unsigned long long bits(int lo, int hi) { return ((1ull << (hi + 1)) - 1ull) & ~((1ull << lo) - 1ull); }
constexpr long long kAnyCount = std::numeric_limits<int>::max();

// The hooks: what is more than a plain store.  A hook runs behind the row's checks and barrier and ahead of the store;
// an error leaves the field as it was.
static int opt_records(fdm_engine* e, int v) {  // repack (or unpack) the estimator's layers now
  e->opt.records = v;
  return e->estimator_ready ? activate_records(e, e->cfg.estimation_type == 1 ? 1 : 0) : FDM_OK;
}
static int opt_dense(fdm_engine* e, int v) {  // force stamp-gated (0) or dense (1) update sweeps
  e->S.dense = v;
  e->obst_dense_pending = true;  // stamps were not maintained while dense
  e->obst_owe_armed = false;
  return FDM_OK;
}
static int opt_dbg_timeline(fdm_engine* e, int v) {  // measurement only: block start / end ticks of the fused tiled launches
  if (e->d_timeline) { (void)hipFree(e->d_timeline); e->d_timeline = nullptr; }
  e->timeline_cap = 0;
  if (v > 0) {
    e->timeline_cap = 1u << 16;
    HIPCK(hipMalloc(reinterpret_cast<void**>(&e->d_timeline), size_t(e->timeline_cap) * 16));
    HIPCK(hipMemset(e->d_timeline, 0, size_t(e->timeline_cap) * 16));
  }
  return FDM_OK;
}
static int opt_tiled_min(fdm_engine* e, int) {  // set by hand: no map-size condition (enqueue_scan)
  e->tiled_forced = true;
  return FDM_OK;
}

struct OptionRow {
  const char* name;
  int EngineOptions::*field;  // null: the hook is all there is to it
  OptRule rule;
  bool sync;                  // sync_all ahead of the write (every option joins the streams first)
  int (*hook)(fdm_engine*, int);
};
// In the order of EngineOptions' fields (fdm_engine_host.hpp, where each option is documented) and of the list in
// include/fdm_engine.h, which tests/test_option_table.py holds against this table.
static const OptionRow kOptions[] = {
  // the scan path
  {"wave_merge", &EngineOptions::wave_merge, opt_bool(), false, nullptr},
  {"bin_variant", &EngineOptions::bin_variant, opt_one_of(1 | 2 | 16, "0, 1 or 4"), false, nullptr},
  {"overlap", &EngineOptions::overlap, opt_bool(), false, nullptr},
  {"zero_copy", &EngineOptions::zero_copy, opt_range(0, kAnyCount, "a point count (0 = off)"), false, nullptr},
  {"records", &EngineOptions::records, opt_bool(), false, opt_records},
  {"dense", nullptr, opt_bool(), false, opt_dense},
  {"move_clear_basic", &EngineOptions::move_clear_basic, opt_bool(), true, nullptr},
  // the large-scan pipeline
  {"tiled", &EngineOptions::tiled, opt_bool(), false, nullptr},
  {"tiled_min", &EngineOptions::tiled_min, opt_range(0, kAnyCount, "a point count"), false, opt_tiled_min},
  // the batch pipeline
  {"batch", &EngineOptions::batch, opt_bool(), false, nullptr},
  {"batch_max", &EngineOptions::batch_max, opt_one_of(1 | bits(2, kMaxBatch), "0 (automatic) or 2 .. 32 scans per launch"), false, nullptr},
  {"batch_fuse", &EngineOptions::batch_fuse, opt_bool(), false, nullptr},
  {"batch_crop", &EngineOptions::batch_crop, opt_bool(), false, nullptr},
  {"batch_walk", &EngineOptions::batch_walk, opt_range(-1, 1, "-1 (automatic), 0, 1"), false, nullptr},
  {"batch_ray", &EngineOptions::batch_ray, opt_bool(), false, nullptr},
  {"batch_ray_seg", &EngineOptions::batch_ray_seg, opt_one_of(bits(1, 1) | bits(4, 4) | bits(8, 8) | bits(16, 16), "1, 4, 8 or 16 lanes per ray"), false, nullptr},
  {"batch_ray_lds", &EngineOptions::batch_ray_lds, opt_bool(), false, nullptr},
  {"batch_ray_parts", &EngineOptions::batch_ray_parts, opt_range(0, 64, "0 (automatic) .. 64"), false, nullptr},
  // the raycasting stage.  (Its options are read when a scan's stage is LAUNCHED; a held-back stage of the previous scan
  // may still be pending: the join every option starts with sends it off first, so that a switch never lands in the scan
  // before it — results are the same either way, A/B timings are attributed to the right scan)
  {"voxel_small", &EngineOptions::voxel_small, opt_bool(), false, nullptr},
  {"voxel_small_max", &EngineOptions::voxel_small_max, opt_range(1, 1 << 20, "1 .. 2^20 points"), false, nullptr},
  {"voxel_any_order", &EngineOptions::voxel_any_order, opt_range(0, 1, "0 (stable), 1 (std::sort)"), true, nullptr},
  {"ray_large_min", &EngineOptions::ray_large_min, opt_at_least(1), false, nullptr},
  {"ray_wedge", &EngineOptions::ray_wedge, opt_bool(), false, nullptr},
  {"ray_overlap", &EngineOptions::ray_overlap, opt_range(-1, 1, "-1 (automatic), 0, 1"), true, nullptr},
  // measurement only
  {"dbg_batch", &EngineOptions::dbg_batch, opt_raw(), false, nullptr},
  {"dbg_ray", &EngineOptions::dbg_ray, opt_raw(), false, nullptr},
  {"dbg_timeline", nullptr, opt_raw(), true, opt_dbg_timeline},
};

/* tuning knobs of the A/B measurements (not part of the reference surface): include/fdm_engine.h lists them */
int fdm_engine_set_option(fdm_engine* e, const char* key, int value) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !key) return fail(FDM_ERR_INVALID, "null argument");
  for (const OptionRow& o : kOptions) {
    if (std::strcmp(key, o.name) != 0) continue;
    const OptRule& r = o.rule;
    bool ok = true;
    switch (r.kind) {
      case OptRule::kBool: value = value != 0; break;
      case OptRule::kRaw: break;
      case OptRule::kAtLeast: value = int(std::max<long long>(value, r.a)); break;
      case OptRule::kRange: ok = value >= r.a && value <= r.b; break;
      case OptRule::kOneOf: ok = value >= 0 && value < 64 && ((r.a >> value) & 1); break;
    }
    if (!ok) return fail(FDM_ERR_INVALID, std::string(o.name) + ": " + r.accepts);
    if (o.sync) if (int rc = sync_all(e)) return rc;
    if (o.hook) if (int rc = o.hook(e, value)) return rc;
    if (o.field) e->opt.*o.field = value;
    return FDM_OK;
  }
  return fail(FDM_ERR_INVALID, std::string("unknown option ") + key);
}
