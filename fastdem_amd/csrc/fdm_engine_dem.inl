// fdm_engine_dem.inl — host side of buildDEM (pcd_convert.cpp:275-323) and of its two filter stages: statistical outlier
// removal (fdm_knn.hpp; nanoPCL outlier_removal_impl.hpp:83-142) and floating-point removal (fdm_dem.hpp).
// Part of fdm_engine_post.hip, behind fdm_engine_cloud.inl (DevBuf, Events, the cloud staging, map_over_cloud) and
// fdm_engine_raster.inl (whole_map, the rasterization entry), whose helpers it uses.  Offline calls: synchronous, scratch
// is allocated per call and freed on return; the stages before a map exists run on the null stream.

namespace {
// the two sides of a radix sort of n (key, index) pairs and its histograms (fdm_rsort.hpp), in one allocation
struct SortBufs {
  DevBuf mem;
  RsPairs<uint32_t> pairs{};
  int alloc(unsigned n) {
    const size_t cap = cloud_stride(n);
    if (int rc = mem.alloc((4 * cap + rs_hist_words(n)) * sizeof(uint32_t))) return rc;
    uint32_t* const b = mem.as<uint32_t>();
    pairs = {{b, b + cap}, {b + 2 * cap, b + 3 * cap}, b + 4 * cap};
    return FDM_OK;
  }
};

thread_local fdm_sor_stats g_sor_stats = {};

// effective_k (outlier_removal_impl.hpp:90) or 0 where the reference returns an empty cloud (:86, :91)
uint64_t sor_effective_k(uint64_t n, int k) {
  if (n < 2 || k == 0) return 0;
  return k < 0 ? n - 1 : std::min<uint64_t>(uint64_t(k), n - 1);  // (a negative int converts to a huge size_t)
}

// The column size: about `per` = max(4, k / 2) points per column were the cloud spread evenly over its x / y bounding
// box (a real cloud is denser where it has points: more per occupied column, never fewer), and at most kKnnGridMax
// columns per axis.  A box without area (a line of points, one point repeated) falls back to the points per length, then
// to one column.
KnnGrid sor_grid(float min_x, float min_y, float max_x, float max_y, uint64_t n, unsigned k) {
  const double ex = double(max_x) - double(min_x), ey = double(max_y) - double(min_y);
  const double per = std::max(4.0, 0.5 * double(k));
  double h = std::sqrt(per * ex * ey / double(n));
  if (!(h > 0.0)) h = per * std::max(ex, ey) / double(n);
  h = std::max(h, std::max(ex, ey) / double(kKnnGridMax - 1u));
  KnnGrid G{};
  G.min_x = min_x;
  G.min_y = min_y;
  G.h = float(h);
  G.inv_h = 1.0f / G.h;
  if (!(G.h > 0.0f) || !std::isfinite(G.h) || !std::isfinite(G.inv_h) || !(G.inv_h > 0.0f)) { G.h = 1.0f; G.inv_h = 1.0f; }
  // the column of the box's far corner, by the device's own arithmetic (knn_u / knn_col)
  auto cols = [&](float mx, float mn) {
    const float u = (mx - mn) * G.inv_h;
    const double c = std::isfinite(u) && u > 0.0f ? std::floor(double(u)) : 0.0;
    return int(std::min(c, double(kKnnGridMax - 1u))) + 1;
  };
  G.gx = cols(max_x, min_x);
  G.gy = cols(max_y, min_y);
  return G;
}

// The k-NN search grid of n device points (fdm_knn.hpp): the column size picked for k, the points in column order and the
// table of column starts, with the counters and the queue the search kernels fill.  Outlier removal and normal estimation
// (fdm_engine_normals.inl) search the same grid.
struct KnnIndex {
  DevBuf b_stat, b_pts, b_start, b_queue;
  SortBufs S;
  KnnGrid G{};
  KnnStat* st() const { return b_stat.as<KnnStat>(); }
  const float4* pts() const { return b_pts.as<float4>(); }
  const uint32_t* start() const { return b_start.as<uint32_t>(); }
  uint32_t* queue() const { return b_queue.as<uint32_t>(); }
};
// bounds (and the refusal of a coordinate that is not finite), keys, sort, gather, starts.  Synchronises s once, for the
// bounding box.
int knn_grid_build(hipStream_t s, unsigned n, const float* dx, const float* dy, const float* dz, unsigned k, KnnIndex& I) {
  if (int rc = I.b_stat.alloc(sizeof(KnnStat))) return rc;
  KnnStat* const st = I.st();
  const unsigned blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_knn_init, dim3(1), dim3(64), 0, s, st);
  hipLaunchKernelGGL(k_knn_bounds, dim3(std::min(blocks, 2048u)), dim3(256), 0, s, n, dx, dy, dz, st);
  HIPCK(hipGetLastError());
  KnnStat hs{};
  HIPCK(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (hs.nonfinite)
    return fail(FDM_ERR_INVALID, "the cloud has a coordinate that is not finite (undefined in the reference's k-d tree)");
  I.G = sor_grid(unord_host(hs.min_x), unord_host(hs.min_y), unord_host(hs.max_x), unord_host(hs.max_y), n, k);
  const KnnGrid& G = I.G;
  const unsigned ncol = unsigned(G.gx) * unsigned(G.gy);
  SortBufs& S = I.S;
  if (int rc = S.alloc(n)) return rc;
  if (int rc = I.b_pts.alloc(size_t(n) * sizeof(float4))) return rc;
  if (int rc = I.b_start.alloc((size_t(ncol) + 1) * sizeof(uint32_t))) return rc;
  if (int rc = I.b_queue.alloc(size_t(n) * sizeof(uint32_t))) return rc;
  hipLaunchKernelGGL(k_knn_keys, dim3(blocks), dim3(256), 0, s, n, dx, dy, G, S.pairs.keys[0]);
  const int side = rs_enqueue(s, S.pairs, n, rs_key_bits(ncol - 1u));
  hipLaunchKernelGGL(k_knn_gather, dim3(blocks), dim3(256), 0, s, n, S.pairs.idx[side], dx, dy, dz, I.b_pts.as<float4>());
  hipLaunchKernelGGL(k_knn_starts, dim3((ncol + 1u + 255u) / 256u), dim3(256), 0, s, n, S.pairs.keys[side], ncol,
                     I.b_start.as<uint32_t>());
  HIPCK(hipGetLastError());
  return FDM_OK;
}
// the top-k bucket (KB of the search kernels) that holds k
int knn_bucket(int k) { return k <= 4 ? 4 : (k <= 16 ? 16 : (k <= 32 ? 32 : 64)); }

template <int KB>
void sor_search(hipStream_t s, unsigned n, int k, const float4* pts, const uint32_t* start, const KnnGrid& G,
                float* mean, uint32_t* queue, KnnStat* st) {
  hipLaunchKernelGGL((k_knn_search<KB>), dim3((n + 255u) / 256u), dim3(256), 0, s, n, k, pts, start, G, mean, queue, st);
}
template <int KB>
void sor_brute(hipStream_t s, unsigned nq, unsigned n, int k, const uint32_t* queue, const float4* pts, float* mean) {
  hipLaunchKernelGGL((k_knn_brute<KB>), dim3(nq), dim3(kKnnBruteThreads), 0, s, queue, n, k, pts, mean);
}

// SOR of n >= 2 device points with 1 <= k <= min(64, n - 1): d_mean[n] and d_keep[n] are filled, *threshold and *n_kept
// set, g_sor_stats left for fdm_sor_last_stats.  Synchronous on stream s.
int sor_device(hipStream_t s, unsigned n, const float* dx, const float* dy, const float* dz, int k, float std_mul,
               float* d_mean, uint8_t* d_keep, float* threshold, uint64_t* n_kept) {
  g_sor_stats = fdm_sor_stats{};
  g_sor_stats.n_queries = n;
  Events E;
  if (int rc = E.init(6)) return rc;
  const unsigned blocks = (n + 255u) / 256u;
  HIPCK(hipEventRecord(E.ev[0], s));
  KnnIndex I;
  if (int rc = knn_grid_build(s, n, dx, dy, dz, unsigned(k), I)) return rc;
  KnnStat* const st = I.st();
  KnnStat hs{};
  const KnnGrid& G = I.G;
  g_sor_stats.grid_x = G.gx;
  g_sor_stats.grid_y = G.gy;
  g_sor_stats.voxel = G.h;
  const DevBuf &b_pts = I.b_pts, &b_start = I.b_start, &b_queue = I.b_queue;
  HIPCK(hipEventRecord(E.ev[1], s));
  const int bucket = knn_bucket(k);
  switch (bucket) {
    case 4: sor_search<4>(s, n, k, b_pts.as<float4>(), b_start.as<uint32_t>(), G, d_mean, b_queue.as<uint32_t>(), st); break;
    case 16: sor_search<16>(s, n, k, b_pts.as<float4>(), b_start.as<uint32_t>(), G, d_mean, b_queue.as<uint32_t>(), st); break;
    case 32: sor_search<32>(s, n, k, b_pts.as<float4>(), b_start.as<uint32_t>(), G, d_mean, b_queue.as<uint32_t>(), st); break;
    default: sor_search<64>(s, n, k, b_pts.as<float4>(), b_start.as<uint32_t>(), G, d_mean, b_queue.as<uint32_t>(), st); break;
  }
  HIPCK(hipGetLastError());
  HIPCK(hipEventRecord(E.ev[2], s));
  HIPCK(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  const unsigned nq = hs.n_queue;
  if (nq > n) return fail(FDM_ERR_HIP, "k-NN queue overran the cloud");
  g_sor_stats.n_fallback = nq;
  if (nq) {
    switch (bucket) {
      case 4: sor_brute<4>(s, nq, n, k, b_queue.as<uint32_t>(), b_pts.as<float4>(), d_mean); break;
      case 16: sor_brute<16>(s, nq, n, k, b_queue.as<uint32_t>(), b_pts.as<float4>(), d_mean); break;
      case 32: sor_brute<32>(s, nq, n, k, b_queue.as<uint32_t>(), b_pts.as<float4>(), d_mean); break;
      default: sor_brute<64>(s, nq, n, k, b_queue.as<uint32_t>(), b_pts.as<float4>(), d_mean); break;
    }
    HIPCK(hipGetLastError());
  }
  HIPCK(hipEventRecord(E.ev[3], s));
  // the two global sums, fp64, in input order (outlier_removal_impl.hpp:118-129): on the host, after one download
  std::vector<float> means(n);
  HIPCK(hipMemcpyAsync(means.data(), d_mean, size_t(n) * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  double sum = 0.0;
  for (unsigned i = 0; i < n; ++i) sum += means[i];
  const double global_mean = sum / double(n);
  double sum_sq_diff = 0.0;
  for (unsigned i = 0; i < n; ++i) {
    const double diff = means[i] - global_mean;
    sum_sq_diff += diff * diff;
  }
  const float global_std = float(std::sqrt(sum_sq_diff / double(n)));
  const float thr = float(global_mean) + std_mul * global_std;
  hipLaunchKernelGGL(k_sor_keep, dim3(blocks), dim3(256), 0, s, n, d_mean, thr, d_keep, st);
  HIPCK(hipGetLastError());
  HIPCK(hipEventRecord(E.ev[4], s));
  HIPCK(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  *threshold = thr;
  *n_kept = hs.n_kept;
  for (int q = 0; q < 4; ++q) g_sor_stats.ms[q] = E.ms(q, q + 1);
  return FDM_OK;
}

// keep[i] of n device points on e's geometry; synchronous on e's stream
int height_filter_device(fdm_engine* e, unsigned n, const float* dx, const float* dy, const float* dz,
                         float height_threshold, float bin, uint8_t* d_keep, uint64_t* n_kept) {
  int rc;
  if ((rc = resolve_pending(e))) return rc;
  hipStream_t s = e->stream;
  const uint32_t ncell = uint32_t(e->ncell);
  const unsigned blocks = (n + 255u) / 256u;
  const int slot = int(e->scan_no & 3);
  DevBuf b_stat, b_rstat, b_cell, b_bins, b_cmin, b_cmax;
  SortBufs S;
  if ((rc = b_stat.alloc(sizeof(DemStat)))) return rc;
  if ((rc = b_rstat.alloc(sizeof(RasterStat)))) return rc;
  if ((rc = b_cell.alloc(size_t(n) * sizeof(uint32_t)))) return rc;
  if ((rc = b_bins.alloc(size_t(n) * sizeof(uint32_t)))) return rc;
  if ((rc = b_cmin.alloc(size_t(ncell) * sizeof(uint32_t)))) return rc;
  if ((rc = b_cmax.alloc(size_t(ncell) * sizeof(uint32_t)))) return rc;
  if ((rc = S.alloc(n))) return rc;
  DemStat* const st = b_stat.as<DemStat>();
  uint32_t* const cell = b_cell.as<uint32_t>();
  uint32_t* const bins = b_bins.as<uint32_t>();
  uint32_t* const cmin = b_cmin.as<uint32_t>();
  uint32_t* const cmax = b_cmax.as<uint32_t>();
  const unsigned fill_blocks = unsigned(std::min<size_t>((size_t(ncell) + 255) / 256, 4096));
  hipLaunchKernelGGL(k_dem_stat_init, dim3(1), dim3(64), 0, s, st);
  hipLaunchKernelGGL(k_ras_stat_init, dim3(1), dim3(64), 0, s, b_rstat.as<RasterStat>());
  hipLaunchKernelGGL(k_fill_u32, dim3(fill_blocks), dim3(256), 0, s, cmin, 0xFFFFFFFFu, size_t(ncell));
  hipLaunchKernelGGL(k_fill_u32, dim3(fill_blocks), dim3(256), 0, s, cmax, 0u, size_t(ncell));
  hipLaunchKernelGGL(k_ras_ids, dim3(blocks), dim3(256), 0, s, n, dx, dy, dz, e->G, e->d_state, slot, ncell, cell,
                     b_rstat.as<RasterStat>());
  hipLaunchKernelGGL(k_hf_minmax, dim3(blocks), dim3(256), 0, s, n, cell, dz, ncell, cmin, cmax);
  hipLaunchKernelGGL(k_hf_bins, dim3(blocks), dim3(256), 0, s, n, cell, dz, ncell, cmin, cmax, bin, bins, st);
  HIPCK(hipGetLastError());
  DemStat hs{};
  HIPCK(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
  if ((rc = sync_all(e))) return rc;
  if (hs.bad)
    return fail(FDM_ERR_INVALID, "a cell's z range over the bin size does not fit an int32 (undefined in the reference)");
  // by bin, then (stable) by cell: the pairs end up ordered by (cell, bin, index)
  const RsPairs<uint32_t>& B = S.pairs;
  HIPCK(hipMemcpyAsync(B.keys[0], bins, size_t(n) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  const int side1 = rs_enqueue(s, B, n, rs_key_bits(hs.max_bin));
  if (side1 != 0) HIPCK(hipMemcpyAsync(B.idx[0], B.idx[side1], size_t(n) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_dem_gather_u32, dim3(blocks), dim3(256), 0, s, n, B.idx[0], cell, B.keys[0]);
  const int side2 = rs_enqueue(s, B, n, rs_key_bits(ncell), 0, kRsIdxGiven);
  hipLaunchKernelGGL(k_hf_peak, dim3(blocks), dim3(256), 0, s, n, B.keys[side2], B.idx[side2], ncell, bins, cmin, bin,
                     height_threshold, cmax);
  hipLaunchKernelGGL(k_hf_keep, dim3(blocks), dim3(256), 0, s, n, cell, dz, ncell, cmax, d_keep, st);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
  if ((rc = sync_all(e))) return rc;
  *n_kept = hs.n_kept;
  return FDM_OK;
}

// the kept points of five channels (ch[k] nullptr = absent) into out[k], in input order; *n_out = how many.  Synchronous.
int compact_device(hipStream_t s, unsigned n, const uint8_t* d_keep, const float* const ch[5], float* const out[5]) {
  const unsigned blocks = (n + 255u) / 256u;
  DevBuf b_counts;
  if (int rc = b_counts.alloc((size_t(blocks) + 1) * sizeof(uint32_t))) return rc;
  DemChannels C{};
  for (int k = 0; k < 5; ++k) { C.in[k] = ch[k]; C.out[k] = out[k]; }
  hipLaunchKernelGGL(k_dem_count, dim3(blocks), dim3(256), 0, s, n, d_keep, b_counts.as<uint32_t>());
  hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, s, b_counts.as<uint32_t>(), blocks);
  hipLaunchKernelGGL(k_dem_compact, dim3(blocks), dim3(256), 0, s, n, d_keep, b_counts.as<uint32_t>(), C);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(s));
  return FDM_OK;
}
}  // namespace

extern "C" {

void fdm_default_dem_config(fdm_dem_config* c) {  // DEMConfig{} (io/pcd_convert.hpp:28-42)
  if (!c) return;
  c->resolution = 0.1f;
  c->method = 0;
  c->sor_k = 10;
  c->sor_std_mul = 1.0f;
  c->height_threshold = 2.0f;
  c->bin_size = 0.0f;
  c->inpaint_iterations = 3;
}

int fdm_sor_last_stats(fdm_sor_stats* out) {
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  *out = g_sor_stats;
  return FDM_OK;
}

int fdm_statistical_outlier_removal(uint64_t n, const float* x, const float* y, const float* z, int on_device, int k,
                                    float std_mul, int device, uint8_t* keep, float* mean_dist, float* threshold,
                                    uint64_t* n_kept) {
  if (!keep || !threshold || !n_kept) return fail(FDM_ERR_INVALID, "null argument");
  *threshold = 0.0f;
  *n_kept = 0;
  g_sor_stats = fdm_sor_stats{};
  if (int rc = check_cloud(n, x, y, z)) return rc;
  const uint64_t k_eff = sor_effective_k(n, k);
  if (k_eff > uint64_t(kKnnMaxK)) return fail(FDM_ERR_INVALID, "statistical outlier removal takes at most 64 neighbours");
  if (n == 0) return FDM_OK;
  if (int rc = pick_device(device)) return rc;
  const unsigned np = unsigned(n);
  if (k_eff == 0) {  // k == 0, one point: nothing is kept
    if (on_device) {
      HIPCK(hipMemset(keep, 0, size_t(n)));
      if (mean_dist) HIPCK(hipMemset(mean_dist, 0, size_t(n) * sizeof(float)));
    } else {
      std::memset(keep, 0, size_t(n));
      if (mean_dist) std::memset(mean_dist, 0, size_t(n) * sizeof(float));
    }
    return FDM_OK;
  }
  CloudBlock b_in;
  DevBuf b_mean, b_keep;
  const void* const src[3] = {x, y, z};
  const float* d[3];
  if (int rc = stage_cloud(nullptr, n, 3, src, on_device != 0, b_in, d)) return rc;
  float* d_mean = mean_dist;
  uint8_t* d_keep = keep;
  if (!on_device || !mean_dist) {
    if (int rc = b_mean.alloc(size_t(n) * sizeof(float))) return rc;
    d_mean = b_mean.as<float>();
  }
  if (!on_device) {
    if (int rc = b_keep.alloc(size_t(n))) return rc;
    d_keep = b_keep.as<uint8_t>();
  }
  if (int rc = sor_device(nullptr, np, d[0], d[1], d[2], int(k_eff), std_mul, d_mean, d_keep, threshold, n_kept)) return rc;
  if (!on_device) {
    HIPCK(hipMemcpy(keep, d_keep, size_t(n), hipMemcpyDeviceToHost));
    if (mean_dist) HIPCK(hipMemcpy(mean_dist, d_mean, size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
  }
  return FDM_OK;
}

int fdm_engine_remove_floating_points(fdm_engine* e, uint64_t n, const float* x, const float* y, const float* z,
                                      int on_device, float height_threshold, float bin_size, uint8_t* keep,
                                      uint64_t* n_kept) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !keep || !n_kept) return fail(FDM_ERR_INVALID, "null argument");
  *n_kept = 0;
  if (!whole_map(e)) return fail(FDM_ERR_INVALID, "removeFloatingPoints is not defined for tiled engines");
  if (int rc = check_cloud(n, x, y, z)) return rc;
  const float bin = bin_size > 0.0f ? bin_size : float(e->G.res);  // pcd_convert.cpp:308-309
  if (!(bin > 0.0f) || !std::isfinite(bin)) return fail(FDM_ERR_INVALID, "the bin size must be positive");
  if (n == 0) return FDM_OK;
  HIPCK(hipSetDevice(e->device));
  CloudBlock b_in;
  DevBuf b_keep;
  const void* const src[3] = {x, y, z};
  const float* d[3];
  if (int rc = stage_cloud(e->stream, n, 3, src, on_device != 0, b_in, d)) return rc;
  uint8_t* d_keep = keep;
  if (!on_device) {
    if (int rc = b_keep.alloc(size_t(n))) return rc;
    d_keep = b_keep.as<uint8_t>();
  }
  if (int rc = height_filter_device(e, unsigned(n), d[0], d[1], d[2], height_threshold, bin, d_keep, n_kept)) return rc;
  if (!on_device) {
    HIPCK(hipMemcpyAsync(keep, d_keep, size_t(n), hipMemcpyDeviceToHost, e->stream));
    return sync_all(e);
  }
  return FDM_OK;
}

// buildDEM(cloud, config): pcd_convert.cpp:275-323
int fdm_engine_build_dem(uint64_t n, const void* x, const void* y, const void* z, const void* intensity, const void* rgb,
                         int on_device, const fdm_dem_config* cfg, int device, fdm_engine** out_engine,
                         fdm_dem_stats* stats) {
  fdm_dem_stats local{};
  fdm_dem_stats& S = stats ? *stats : local;
  S = fdm_dem_stats{};
  S.n_input = n;
  if (!out_engine) return fail(FDM_ERR_INVALID, "null argument");
  *out_engine = nullptr;
  fdm_dem_config c;
  fdm_default_dem_config(&c);
  if (cfg) c = *cfg;
  if (n == 0) return FDM_SKIP_EMPTY_CLOUD;  // :276 `return {}`: no map
  if (int rc = check_cloud(n, x, y, z, c.method)) return rc;
  if (int rc = check_resolution(c.resolution)) return rc;
  const float bin = c.bin_size > 0.0f ? c.bin_size : c.resolution;  // :308-309
  if (!std::isfinite(bin)) return fail(FDM_ERR_INVALID, "the bin size must be finite");
  const uint64_t k_eff = sor_effective_k(n, c.sor_k);
  if (k_eff > uint64_t(kKnnMaxK)) return fail(FDM_ERR_INVALID, "statistical outlier removal takes at most 64 neighbours");
  if (k_eff == 0) return FDM_SKIP_ALL_FILTERED;  // :282: SOR returned an empty cloud
  if (int rc = pick_device(device)) return rc;
  const unsigned np = unsigned(n);
  Events E;
  if (int rc = E.init(8)) return rc;
  // 0. the cloud on the device
  const void* const src[5] = {x, y, z, intensity, rgb};
  const float* ch[5];
  CloudBlock b_stage;
  if (int rc = stage_cloud(nullptr, n, 5, src, on_device != 0, b_stage, ch)) return rc;
  // 1. statistical outlier removal (:279-282)
  DevBuf b_mean, b_keep;
  CloudBlock b_a;
  if (int rc = b_mean.alloc(size_t(n) * sizeof(float))) return rc;
  if (int rc = b_keep.alloc(size_t(n))) return rc;
  if (int rc = sor_device(nullptr, np, ch[0], ch[1], ch[2], int(k_eff), c.sor_std_mul, b_mean.as<float>(),
                          b_keep.as<uint8_t>(), &S.sor_threshold, &S.n_after_sor))
    return rc;
  S.n_sor_fallback = g_sor_stats.n_fallback;
  for (int q = 0; q < 4; ++q) S.stage_ms[q] = g_sor_stats.ms[q];
  if (S.n_after_sor == 0) return FDM_SKIP_ALL_FILTERED;
  const unsigned n1 = unsigned(S.n_after_sor);
  if (int rc = b_a.alloc(n1, 5)) return rc;
  const float* a[5];
  float* a_out[5];
  for (int q = 0; q < 5; ++q) {
    a_out[q] = b_a.ch(q);
    a[q] = ch[q] ? a_out[q] : nullptr;
  }
  if (int rc = compact_device(nullptr, np, b_keep.as<uint8_t>(), ch, a_out)) return rc;
  // 2. the map over the survivors' bounding box (:285-305)
  fdm_engine* e = nullptr;
  if (int rc = map_over_cloud(n1, a[0], a[1], c.resolution, device, &e)) return rc;
  auto drop = [&](int rc) { fdm_engine_destroy(e); return rc; };
  // 3. floating-point removal (:308-311)
  DevBuf b_keep2;
  CloudBlock b_b;
  if (int rc = b_keep2.alloc(size_t(n1))) return drop(rc);
  (void)hipEventRecord(E.ev[0], e->stream);
  if (int rc = height_filter_device(e, n1, a[0], a[1], a[2], c.height_threshold, bin, b_keep2.as<uint8_t>(),
                                    &S.n_after_height))
    return drop(rc);
  const unsigned n2 = unsigned(S.n_after_height);
  if (int rc = b_b.alloc(n2, 5)) return drop(rc);
  const float* b[5];
  float* b_out[5];
  for (int q = 0; q < 5; ++q) {
    b_out[q] = b_b.ch(q);
    b[q] = a[q] ? b_out[q] : nullptr;
  }
  if (n2)
    if (int rc = compact_device(e->stream, n1, b_keep2.as<uint8_t>(), a, b_out)) return drop(rc);
  (void)hipEventRecord(E.ev[1], e->stream);
  // 4. rasterization (:314; an empty cloud leaves the map as it is), 5. inpainting (:317-320)
  if (n2) {
    const int rc = fdm_engine_from_point_cloud_device(e, n2, b[0], b[1], b[2], b[3],
                                                      reinterpret_cast<const uint32_t*>(b[4]), c.method, &S.raster);
    if (rc < 0) return drop(rc);
  }
  (void)hipEventRecord(E.ev[2], e->stream);
  if (c.inpaint_iterations > 0) {
    const int rc = fdm_engine_apply_inpainting(e, c.inpaint_iterations, 2, 1);
    if (rc < 0) return drop(rc);
  }
  (void)hipEventRecord(E.ev[3], e->stream);
  if (int rc = sync_all(e)) return drop(rc);
  for (int q = 0; q < 3; ++q) S.stage_ms[4 + q] = E.ms(q, q + 1);
  *out_engine = e;
  return FDM_OK;
}

}  // extern "C"
