// fdm_engine_post.inl — host side of the stencil post-processing stages (kernels: fdm_post.hpp).
// Part of fdm_engine_post.hip (one of the library's five translation units, fdm_engine_host.hpp).

extern "C" {

// ---- stencil post-processing ----
namespace {
// Spatial tiles: a stencil that reaches `need` cells is exact on the owned cells iff every window side
// that is not a map side carries a halo at least that wide.
int check_halo(const fdm_engine* e, int need) {
  const GeomConst& G = e->G;
  const int top = G.o_r0 - G.s_r0, left = G.o_c0 - G.s_c0;
  const int bottom = (G.s_r0 + G.s_rows) - (G.o_r0 + G.o_rows), right = (G.s_c0 + G.s_cols) - (G.o_c0 + G.o_cols);
  const bool ok = (G.s_r0 == 0 || top >= need) && (G.s_c0 == 0 || left >= need) &&
                  (G.s_r0 + G.s_rows == G.rows || bottom >= need) && (G.s_c0 + G.s_cols == G.cols || right >= need);
  if (!ok) return fail(FDM_ERR_INVALID, "tile halo narrower than the stencil (" + std::to_string(need) + " cells needed)");
  return FDM_OK;
}
// neighbourhood offsets, dr-major / dc-minor; box = region(Size(k,k)), disc = region(radius)
int upload_region(fdm_engine* e, const std::vector<RegionEntry>& reg) {
  // (any disc the reference accepts: 0.3 m on a 0.02 m map is 707 cells)
  if (int rc_grow = grow_device(e, &e->d_region, &e->region_cap, reg.size(),
                                std::max<size_t>(size_t(kMaxRegion), reg.size() + reg.size() / 4)))
    return rc_grow;
  // the table of the last call stays on the device: a stage called again with the same parameters (the usual case: once
  // per published map) uploads nothing and waits for nothing
  if (e->h_region.size() == reg.size() && !reg.empty() &&
      std::memcmp(e->h_region.data(), reg.data(), reg.size() * sizeof(RegionEntry)) == 0)
    return FDM_OK;
  e->h_region.clear();
  HIPCK(hipMemcpyAsync(e->d_region, reg.data(), reg.size() * sizeof(RegionEntry), hipMemcpyHostToDevice, e->stream));
  if (int rc_sync = sync_all(e)) return rc_sync;  // `reg` is a host temporary
  e->h_region = reg;
  return FDM_OK;
}
void region_disc(const fdm_engine* e, float radius, std::vector<RegionEntry>& reg) {
  reg.clear();
  const float res = static_cast<float>(e->G.res);
  const int k = static_cast<int>(std::floor(radius / res + 1e-4f));
  const float r2 = radius * radius;
  for (int dr = -k; dr <= k; ++dr)
    for (int dc = -k; dc <= k; ++dc) {
      const float d2 = static_cast<float>(dr * dr + dc * dc) * (res * res);
      if (d2 <= r2 * (1.0f + 1e-5f)) reg.push_back({dr, dc, d2, 0.f});
    }
}
unsigned cell_blocks(const fdm_engine* e) { return unsigned((e->ncell + 255) / 256); }
// The global list pool of the big-neighbourhood kernels (fdm_post.hpp, k_median_big): `per_thread` floats for each of
// the threads in flight.  Returns the number of blocks of `threads` threads to launch.
// The pooled kernels insertion-sort every cell's neighbourhood in global memory: ~ entries^2 / 4 moves per cell.  A call
// is refused when that is more than ~1e13 moves over the map (minutes on the device — effectively a hang):
// 1.44 M cells take neighbourhoods of up to ~5 000 entries (a 71 x 71 median), a 64 M-cell map ~790 (28 x 28).
constexpr double kBigStencilMoves = 1.0e13;
int ensure_pool(fdm_engine* e, size_t per_thread, unsigned threads, unsigned* blocks_out, size_t entries) {
  if (double(entries) * double(entries) * 0.25 * double(e->ncell) > kBigStencilMoves)
    return fail(FDM_ERR_INVALID, "neighbourhood too large for this map: " + std::to_string(entries) + " entries per cell x " +
                                     std::to_string(e->ncell) + " cells would keep the device busy for minutes");
  const size_t want_threads = std::min<size_t>(((e->ncell + threads - 1) / threads) * threads, 16384);
  const size_t floats = want_threads * per_thread;
  if (int rc_grow = grow_device(e, &e->d_post_pool, &e->post_pool_cap, floats, floats)) return rc_grow;
  *blocks_out = unsigned(want_threads / threads);
  return FDM_OK;
}
unsigned tile3_blocks(const fdm_engine* e) {  // 32 x 8-cell tiles of the 3x3 stencils (fdm_post.hpp)
  return unsigned((e->G.s_rows + kS3R - 1) / kS3R) * unsigned((e->G.s_cols + kS3C - 1) / kS3C);
}
int ensure_tmp2(fdm_engine* e) {
  if (!e->d_tmp2) HIPCK(hipMalloc(reinterpret_cast<void**>(&e->d_tmp2), e->ncell * sizeof(float)));
  return FDM_OK;
}
// Every launch site of the four stages names its kernel through this macro: the engine keeps the name, spelled as here,
// for fdm_engine_debug_last_post_kernel (fdm_engine_debug.h) — the tests assert which branch of the dispatch a call took.
#define FDM_POST_KERNEL(...) (e->last_post_kernel = #__VA_ARGS__, (__VA_ARGS__))
}  // namespace

int fdm_engine_apply_inpainting(fdm_engine* e, int max_iterations, int min_valid, int inplace) {
  if (int rc = join_streams(e)) return rc;
  if (!e) return fail(FDM_ERR_INVALID, "null engine");
  e->last_post_kernel = "";  // (a call that returns before it launches leaves the empty name)
  HIPCK(hipSetDevice(e->device));
  int rc;
  if ((rc = check_halo(e, max_iterations > 0 ? max_iterations : 0))) return rc;  // one cell per pass
  if ((rc = resolve_pending(e))) return rc;
  Layer* elev = find_layer(e, "elevation");
  if (!elev) return fail(FDM_ERR_NO_LAYER, "no layer elevation");
  const char* out_name = inplace ? "elevation" : "elevation_inpainted";
  if (!find_layer(e, out_name) && (rc = add_layer(e, out_name, NAN, false))) return rc;
  elev = find_layer(e, "elevation");
  Layer* out = find_layer(e, out_name);
  if ((rc = ensure_tmp(e))) return rc;
  float* A = lptr(e, *out);
  const int As = lstride(e, *out);
  float* B = e->d_tmp;
  const int slot = int(e->scan_no & 3);
  // `inpainted = elevation`, then up to max_iterations passes ping-ponging output layer <-> staging;
  // the reference stops after a pass that changed nothing — further passes are identities, so all
  // of them are simply run.  The copy goes to whichever side makes the LAST pass land in the layer.
  const int iters = max_iterations > 0 ? max_iterations : 0;
  const bool start_in_layer = (iters % 2) == 0;
  if (!inplace || !start_in_layer) {
    if ((rc = copy_strided(e, start_in_layer ? A : B, start_in_layer ? As : 1, lptr(e, *elev), lstride(e, *elev))))
      return rc;
  }
  bool in_layer = start_in_layer;
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_inpaint_pass_tiled), dim3(tile3_blocks(e)), dim3(256), 0, e->stream, e->G, e->d_state, slot,
                       in_layer ? A : B, in_layer ? As : 1, in_layer ? B : A, in_layer ? 1 : As, min_valid);
    in_layer = !in_layer;
  }
  HIPCK(hipGetLastError());
  return FDM_OK;
}

int fdm_engine_apply_spatial_smoothing(fdm_engine* e, const char* layer, int kernel_size, int min_valid) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !layer) return fail(FDM_ERR_INVALID, "null argument");
  e->last_post_kernel = "";  // (a call that returns before it launches leaves the empty name)
  // (any kernel size the reference accepts: region(Size(k, k)) spans dr, dc in [-k/2, k/2] — for an even k that is the
  // (k + 1)-wide box; a window beyond kMaxRegion cells takes the pooled kernel)
  if (kernel_size < 1 || kernel_size > 4096) return fail(FDM_ERR_INVALID, "kernel_size must be in [1, 4096]");
  HIPCK(hipSetDevice(e->device));
  int rc;
  if ((rc = check_halo(e, kernel_size / 2))) return rc;
  if ((rc = resolve_pending(e))) return rc;
  Layer* l = find_layer(e, layer);
  if (!l || l->pending) return FDM_OK;  // spatial_smoothing.hpp:42
  if ((rc = ensure_tmp(e))) return rc;
  if ((rc = copy_strided(e, e->d_tmp, 1, lptr(e, *l), lstride(e, *l)))) return rc;  // the double buffer
  if (kernel_size == 3)
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_median3_tiled), dim3(tile3_blocks(e)), dim3(256), 0, e->stream, e->G, e->d_state,
                       int(e->scan_no & 3), e->d_tmp, lptr(e, *l), lstride(e, *l), min_valid);
  else if ((2 * (kernel_size / 2) + 1) * (2 * (kernel_size / 2) + 1) <= kMaxRegion)
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_median), dim3(cell_blocks(e)), dim3(256), 0, e->stream, e->G, e->d_state,
                       int(e->scan_no & 3), e->d_tmp, lptr(e, *l), lstride(e, *l), kernel_size, min_valid,
                       unsigned(e->ncell));
  else if (median_sel_lds_bytes(kernel_size) <= 160u * 1024u) {
    // selection by bisection on an LDS tile (fdm_post.hpp k_median_sel): every window up to ~175 x 175
    const unsigned lds = median_sel_lds_bytes(kernel_size);
    if ((rc = allow_lds(k_median_sel, lds))) return rc;
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_median_sel), dim3(tile3_blocks(e)), dim3(256), lds, e->stream, e->G, e->d_state, int(e->scan_no & 3),
                       e->d_tmp, lptr(e, *l), lstride(e, *l), kernel_size, min_valid);
  } else {
    const size_t side = size_t(2 * (kernel_size / 2) + 1);
    unsigned blocks = 0;
    if ((rc = ensure_pool(e, side * side, 256u, &blocks, side * side))) return rc;
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_median_big), dim3(blocks), dim3(256), 0, e->stream, e->G, e->d_state, int(e->scan_no & 3),
                       e->d_tmp, lptr(e, *l), lstride(e, *l), kernel_size, min_valid, unsigned(e->ncell), e->d_post_pool);
  }
  HIPCK(hipGetLastError());
  if (std::strcmp(layer, "obstacle") == 0) { e->obst_dense_pending = true; e->obst_owe_armed = false; }
  return FDM_OK;
}

int fdm_engine_apply_uncertainty_fusion(fdm_engine* e, const fdm_fusion_config* cfg) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !cfg) return fail(FDM_ERR_INVALID, "null argument");
  e->last_post_kernel = "";  // (a call that returns before it launches leaves the empty name)
  if (!cfg->enabled) return FDM_OK;
  HIPCK(hipSetDevice(e->device));
  int rc;
  if ((rc = check_halo(e, int(std::floor(cfg->search_radius / static_cast<float>(e->G.res) + 1e-4f))))) return rc;
  if ((rc = resolve_pending(e))) return rc;
  Layer* up = find_layer(e, "upper_bound");
  Layer* lo = find_layer(e, "lower_bound");
  if (!up || !lo) return FDM_OK;  // uncertainty_fusion.cpp:108-113: warn + return
  std::vector<RegionEntry> reg;
  region_disc(e, cfg->search_radius, reg);
  {  // spatial weight of each offset (uncertainty_fusion.cpp:122-123,158): std::exp on a float
    const float inv_2s2 = 1.0f / (2.0f * cfg->spatial_sigma * cfg->spatial_sigma);
    for (auto& r : reg) r.w = std::exp(-r.dist_sq * inv_2s2);
  }
  if ((rc = upload_region(e, reg))) return rc;
  if ((rc = ensure_tmp(e)) || (rc = ensure_tmp2(e))) return rc;
  if (lstride(e, *up) == lstride(e, *lo)) {  // fields of the same cell records (or two dense layers): one pass
    const int blocks = int(std::min<size_t>((e->ncell + 255) / 256, 4096));
    hipLaunchKernelGGL(k_copy_strided2, dim3(blocks), dim3(256), 0, e->stream, e->d_tmp, e->d_tmp2, lptr(e, *up), lptr(e, *lo),
                       lstride(e, *up), e->ncell);
    HIPCK(hipGetLastError());
  } else {
    if ((rc = copy_strided(e, e->d_tmp, 1, lptr(e, *up), lstride(e, *up)))) return rc;
    if ((rc = copy_strided(e, e->d_tmp2, 1, lptr(e, *lo), lstride(e, *lo)))) return rc;
  }
  FusionParams F{};
  F.inv_2s2 = 1.0f / (2.0f * cfg->spatial_sigma * cfg->spatial_sigma);
  F.q_lower = cfg->quantile_lower;
  F.q_upper = cfg->quantile_upper;
  F.min_valid = cfg->min_valid_neighbors;
  F.n_entries = int(reg.size());
  int halo = 0;
  for (const RegionEntry& r : reg) halo = std::max(halo, std::max(std::abs(r.dr), std::abs(r.dc)));
  const auto q_ok = [](float q) { return q >= 1e-6f && q <= 1.0f; };  // (k_fusion_f64_tiled's walk: a positive target within the total)
  if (reg.size() <= 29 && halo <= kFusHaloMax && q_ok(F.q_lower) && q_ok(F.q_upper)) {
    // (a disc of a radius has 1, 5, 9, 13, 21, 25, 29, 37 .. cells: nothing between 29 and 32)
    // samples as doubles sorted by v_min_f64 / v_max_f64 (the default radius: 29 cells), neighbourhood staged in LDS
    const unsigned tblocks = unsigned((e->G.s_rows + kFusTileR - 1) / kFusTileR) *
                             unsigned((e->G.s_cols + kFusTileC - 1) / kFusTileC);
    auto launch_f64 = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(tblocks), dim3(kFusionThreads), fusion_f64_lds_bytes(halo), e->stream, e->G, e->d_state,
                         int(e->scan_no & 3), e->d_region, F, halo, e->d_tmp, e->d_tmp2, lptr(e, *up), lstride(e, *up),
                         lptr(e, *lo), lstride(e, *lo));
    };
    // one instantiation per disc size there is below 30 cells (the sorting network shrinks with it: 171 exchanges for 29
    // samples, 19 for the 9 of the shipped 0.15 m on a 0.1 m map); a disc of one cell: the 29-slot kernel with branches
    const size_t nreg = reg.size();
    if (nreg == 29) launch_f64(FDM_POST_KERNEL(k_fusion_f64_tiled<29, true>));
    else if (nreg == 25) launch_f64(FDM_POST_KERNEL(k_fusion_f64_tiled<25, true>));
    else if (nreg == 21) launch_f64(FDM_POST_KERNEL(k_fusion_f64_tiled<21, true>));
    else if (nreg == 13) launch_f64(FDM_POST_KERNEL(k_fusion_f64_tiled<13, true>));
    else if (nreg == 9) launch_f64(FDM_POST_KERNEL(k_fusion_f64_tiled<9, true>));
    else if (nreg == 5) launch_f64(FDM_POST_KERNEL(k_fusion_f64_tiled<5, true>));
    else launch_f64(FDM_POST_KERNEL(k_fusion_f64_tiled<29, false>));
  } else if (reg.size() <= 32 && halo <= kFusHaloMax) {
    // samples as 64-bit integers sorted in registers, neighbourhood staged in LDS (round 2; any quantile)
    const unsigned tblocks = unsigned((e->G.s_rows + kFusTileR - 1) / kFusTileR) *
                             unsigned((e->G.s_cols + kFusTileC - 1) / kFusTileC);
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_fusion_net32_tiled), dim3(tblocks), dim3(kFusionThreads), 0, e->stream, e->G, e->d_state,
                       int(e->scan_no & 3), e->d_region, F, halo, e->d_tmp, e->d_tmp2, lptr(e, *up), lstride(e, *up),
                       lptr(e, *lo), lstride(e, *lo));
  } else if (int(reg.size()) <= kFusionWaveMax) {  // one wavefront per cell, the samples sorted in LDS
    unsigned n_pad = 64u;
    while (n_pad < reg.size()) n_pad <<= 1;
    const unsigned lds = fusion_wave_lds_bytes(n_pad);
    if ((rc = allow_lds(k_fusion_wave, lds))) return rc;
    const unsigned wblocks = unsigned(std::min<size_t>((e->ncell + 1) / 2, 8192));
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_fusion_wave), dim3(wblocks), dim3(kFusionWaveThreads), lds, e->stream, e->G, e->d_state,
                       int(e->scan_no & 3), e->d_region, F, n_pad, e->d_tmp, e->d_tmp2, lptr(e, *up), lstride(e, *up),
                       lptr(e, *lo), lstride(e, *lo), unsigned(e->ncell));
  } else {  // any radius the reference accepts (config/postprocess.hpp:35)
    unsigned blocks = 0;
    if ((rc = ensure_pool(e, 4 * reg.size(), unsigned(kFusionThreads), &blocks, reg.size()))) return rc;
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_fusion_big), dim3(blocks), dim3(kFusionThreads), 0, e->stream, e->G, e->d_state,
                       int(e->scan_no & 3), e->d_region, F, e->d_tmp, e->d_tmp2, lptr(e, *up), lstride(e, *up),
                       lptr(e, *lo), lstride(e, *lo), unsigned(e->ncell), e->d_post_pool);
  }
  HIPCK(hipGetLastError());
  return FDM_OK;
}

int fdm_engine_apply_feature_extraction(fdm_engine* e, float radius, int min_valid, float lo_pct, float hi_pct) {
  if (int rc = join_streams(e)) return rc;
  if (!e) return fail(FDM_ERR_INVALID, "null engine");
  e->last_post_kernel = "";  // (a call that returns before it launches leaves the empty name)
  HIPCK(hipSetDevice(e->device));
  int rc;
  if ((rc = check_halo(e, int(std::floor(radius / static_cast<float>(e->G.res) + 1e-4f))))) return rc;
  if ((rc = resolve_pending(e))) return rc;
  if (!find_layer(e, "elevation")) return FDM_OK;  // feature_extraction.cpp:33
  const char* names[7] = {"step", "slope", "roughness", "curvature", "_normal_x", "_normal_y", "_normal_z"};
  for (const char* n : names)
    if (!find_layer(e, n) && (rc = add_layer(e, n, NAN, false))) return rc;
  std::vector<RegionEntry> reg;
  region_disc(e, radius, reg);
  FeatureParams F{};
  F.resf = static_cast<float>(e->G.res);
  // the region as k_features_tiled reads it (fdm_post.hpp); uploaded ahead of upload_region's synchronisation
  int halo = 0;
  for (const RegionEntry& r : reg) halo = std::max(halo, std::max(std::abs(r.dr), std::abs(r.dc)));
  std::vector<FeatEntry> tab;
  if (halo <= kFeatHaloMax && reg.size() <= size_t(kMaxRegion)) {
    const int pitch = kFeatTileR + 2 * halo;
    tab.resize(reg.size());
    for (size_t k = 0; k < reg.size(); ++k) {
      FeatEntry& t = tab[k];
      t.off = reg[k].dc * pitch + reg[k].dr;
      t.d0 = static_cast<float>(-reg[k].dr) * F.resf;  // feature_extraction.cpp:74-76
      t.d1 = static_cast<float>(-reg[k].dc) * F.resf;
      t.p00 = t.d0 * t.d0;
      t.p01 = t.d0 * t.d1;
      t.p11 = t.d1 * t.d1;
      t.one = 1.0f;
      t.pad = 0;
    }
    if (!e->d_feat_tab) HIPCK(hipMalloc(reinterpret_cast<void**>(&e->d_feat_tab), kMaxRegion * sizeof(FeatEntry)));
    const bool same_tab = e->h_feat_tab.size() == tab.size() &&
                          std::memcmp(e->h_feat_tab.data(), tab.data(), tab.size() * sizeof(FeatEntry)) == 0;
    if (!tab.empty() && !same_tab) {
      if (int rc_sync = sync_all(e)) return rc_sync;  // (a kernel of an earlier call may still read the old table)
      HIPCK(hipMemcpy(e->d_feat_tab, tab.data(), tab.size() * sizeof(FeatEntry), hipMemcpyHostToDevice));
      e->h_feat_tab = tab;
    }
  }
  Layer* elev = find_layer(e, "elevation");
  F.lo_pct = lo_pct;
  F.hi_pct = hi_pct;
  F.min_valid = min_valid;
  F.n_entries = int(reg.size());
  FeatureOut O{};
  float** outs[7] = {&O.step, &O.slope, &O.roughness, &O.curvature, &O.nx, &O.ny, &O.nz};
  for (int k = 0; k < 7; ++k) *outs[k] = find_layer(e, names[k])->d;
  // order statistics needed by `step`: index lo from the bottom, (count-1-hi) from the top; both grow
  // with count, so the full region bounds them
  const int nmax = int(reg.size());
  const int need_lo = nmax > 0 ? static_cast<int>(lo_pct * float(nmax - 1)) + 1 : 1;
  const int need_hi = nmax > 0 ? (nmax - 1) - static_cast<int>(hi_pct * float(nmax - 1)) + 1 : 1;
  const bool pct_ok = lo_pct >= 0.0f && hi_pct <= 1.0f && lo_pct <= 1.0f && hi_pct >= 0.0f;
  // the stencil reads ~113 neighbours per cell: from a cell-record field (64 B stride) every one of them
  // is its own cache line — a dense copy of the layer first (C4: 0.82 -> see LABNOTES.md, rounds 1-3 §7)
  const float* elev_p = lptr(e, *elev);
  int elev_s = lstride(e, *elev);
  // (the LDS-tiled kernel stages its tile straight from the records: every cell is fetched ~3.4 times, from the L2, behind
  //  other blocks' arithmetic — the copy was 17 of the call's 127 us at configs[3])
  const bool tiled_ok = pct_ok && need_lo <= 16 && need_hi <= 16 && !tab.empty();
  // (the tiled kernel reads its own table only: the plain region — which the fusion stage of the same publish cycle keeps
  //  on the device with its weights — is left alone, and neither stage uploads anything from the second cycle on)
  if (!tiled_ok && (rc = upload_region(e, reg))) return rc;
  if (elev_s != 1 && !tiled_ok) {
    if ((rc = ensure_tmp(e))) return rc;
    if ((rc = copy_strided(e, e->d_tmp, 1, elev_p, elev_s))) return rc;
    elev_p = e->d_tmp;
    elev_s = 1;
  }
  auto launch_feat = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(cell_blocks(e)), dim3(256), 0, e->stream, e->G, e->d_state, int(e->scan_no & 3),
                       e->d_region, F, elev_p, elev_s, O, unsigned(e->ncell));
  };
  // dense layer + a region of bounded reach: LDS-tiled kernel fed from a pre-digested region table (fdm_post.hpp)
  if (tiled_ok) {
    const int rows = e->G.s_rows, cols = e->G.s_cols;
    const unsigned blocks = unsigned((rows + kFeatTileR - 1) / kFeatTileR) * unsigned((cols + kFeatTileC - 1) / kFeatTileC);
    auto launch_tiled = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(kFeatThreads), 0, e->stream, e->G, e->d_state, int(e->scan_no & 3),
                         e->d_feat_tab, F, halo, elev_p, elev_s, O);
    };
    if (need_lo <= 2 && need_hi <= 3) launch_tiled(FDM_POST_KERNEL(k_features_tiled<2, 3>));  // the defaults on a 29-cell disc (0.3 m on a 0.1 m map)
    else if (need_lo <= 4 && need_hi <= 4) launch_tiled(FDM_POST_KERNEL(k_features_tiled<4, 4>));
    else if (need_lo <= 6 && need_hi <= 7) launch_tiled(FDM_POST_KERNEL(k_features_tiled<6, 7>));  // the defaults on a 113-cell disc: 6 from the bottom, 7 from the top
    else if (need_lo <= 8 && need_hi <= 8) launch_tiled(FDM_POST_KERNEL(k_features_tiled<8>));
    else launch_tiled(FDM_POST_KERNEL(k_features_tiled<16>));
  } else if (pct_ok && need_lo <= 8 && need_hi <= 8) launch_feat(FDM_POST_KERNEL(k_features<8>));
  else if (pct_ok && need_lo <= 16 && need_hi <= 16) launch_feat(FDM_POST_KERNEL(k_features<16>));
  else if (features_sel_lds_bytes(halo, int(reg.size())) <= 160u * 1024u) {
    // any disc, any percentile pair: order statistics by bisection on an LDS tile (fdm_post.hpp k_features_sel).
    // Every region of at most kMaxRegion entries comes here, so the pooled kernel below only ever sees larger ones: a
    // disc that reaches h cells holds every offset with dr^2 + dc^2 <= h^2, among them the square of side
    // 2 * floor(h / sqrt(2)) + 1; with at most 256 entries that side is at most 15, so h <= 11 (12 gives side 17).
    static_assert(kMaxRegion < 17 * 17 && 160u * 1024u >= features_sel_lds_bytes(11, kMaxRegion),
                  "a region of <= kMaxRegion entries fits the LDS of k_features_sel");
    const unsigned lds = features_sel_lds_bytes(halo, int(reg.size()));
    if ((rc = allow_lds(k_features_sel, lds))) return rc;
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_features_sel), dim3(tile3_blocks(e)), dim3(256), lds, e->stream, e->G, e->d_state, int(e->scan_no & 3),
                       e->d_region, F, halo, elev_p, O);
  } else {  // any radius the reference accepts (config/postprocess.hpp:45): the sorted heights in the global pool
    unsigned blocks = 0;
    if ((rc = ensure_pool(e, reg.size(), 256u, &blocks, reg.size()))) return rc;
    hipLaunchKernelGGL(FDM_POST_KERNEL(k_features_big), dim3(blocks), dim3(256), 0, e->stream, e->G, e->d_state, int(e->scan_no & 3),
                       e->d_region, F, elev_p, elev_s, O, unsigned(e->ncell), e->d_post_pool);
  }
  HIPCK(hipGetLastError());
  return FDM_OK;
}

int fdm_engine_debug_last_post_kernel(fdm_engine* e, char* out, int cap) {
  if (!e || !out || cap < 1) return fail(FDM_ERR_INVALID, "null argument");
  std::snprintf(out, size_t(cap), "%s", e->last_post_kernel);
  return FDM_OK;
}

}  // extern "C"
