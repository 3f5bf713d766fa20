// fdm_engine_filter.inl — host side of the cloud filters (kernels: fdm_filter.hpp; cropAngle's constants and the work
// bound: fdm_filter_host.hpp): entry points fdm_cloud_radius_outlier_removal, fdm_ror_last_stats and fdm_cloud_crop.
// Part of fdm_engine_post.hip, behind fdm_engine_cluster.inl: the radius outlier removal launches the front half of
// fdm_cloud_cluster (its steps 1 and 2) as it is, without an index list.  Engine-free like the other cloud calls: a call
// picks its device, works on the null stream in scratch of its own and frees it on return.  Synchronous.  Nothing is
// written to the caller's outputs before the last refusal has been decided.

namespace {
thread_local fdm_ror_stats g_ror_stats = {};
}  // namespace

extern "C" {

int fdm_ror_last_stats(fdm_ror_stats* out) {
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  *out = g_ror_stats;
  return FDM_OK;
}

int fdm_cloud_radius_outlier_removal(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                                     float radius, uint64_t min_neighbors, int device,
                                     uint8_t* keep, uint32_t* counts, uint64_t* n_kept) {
  g_ror_stats = fdm_ror_stats{};
  if (!n_kept) return fail(FDM_ERR_INVALID, "null argument");
  *n_kept = 0;
  if (n >= (1ull << 32)) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-1");
  // (the sort counts its tiles of up to 4 096 pairs, and every kernel here its blocks, in 32 bits)
  if (n >= 0xFFFFFFFFull - kRsTile) return fail(FDM_ERR_INVALID, "the cloud has 2^32-4097 points or more");
  if (n && (!x || !y || !z)) return fail(FDM_ERR_INVALID, "null coordinate array");
  if (n && !keep) return fail(FDM_ERR_INVALID, "null argument");
  cluster::Relation R;
  if (!cluster::relation(radius, R))
    return fail(FDM_ERR_INVALID, "radius must be a positive finite number whose voxel range is 1 or 2");
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  hipStream_t s = nullptr;
  const bool host = on_device == 0;
  const unsigned m = unsigned(n), blocks = (m + 255u) / 256u;
  g_ror_stats.n_points = m;
  g_ror_stats.range = R.range;
  if (m == 0) return FDM_OK;

  Events E;
  const bool clock = cloud_profile_on();
  if (clock)
    if (int rc = E.init(6)) return rc;
  auto mark = [&](int k) { return clock ? hipEventRecord(E.ev[k], s) : hipSuccess; };

  CloudBlock b_in;
  const float* d[3] = {nullptr, nullptr, nullptr};
  const void* const src[3] = {x, y, z};
  if (int rc = stage_cloud(s, n, 3, src, !host, b_in, d)) return rc;
  DevBuf b_stat, b_ror, b_pts, b_out;
  SortBufs64 S;
  if (int rc = b_stat.alloc(sizeof(ClusterStat))) return rc;
  if (int rc = b_ror.alloc(sizeof(RorStat))) return rc;
  if (int rc = S.alloc(m)) return rc;
  if (int rc = b_pts.alloc(size_t(m) * sizeof(float4))) return rc;
  ClusterStat* const st = b_stat.as<ClusterStat>();
  RorStat* const rst = b_ror.as<RorStat>();
  float4* const pts = b_pts.as<float4>();
  ClusterStat hs{};
  RorStat hr{};

  // 1. the voxels and what is refused about them (fdm_cloud_cluster's step 1, indices == nullptr)
  HIPCK(mark(0));
  unsigned long long* const vox = S.pairs.keys[1];  // (the sort's other side: free until its first pass)
  hipLaunchKernelGGL(k_cluster_stat_init, dim3(1), dim3(64), 0, s, st);
  hipLaunchKernelGGL(k_cluster_voxels, dim3(blocks), dim3(256), 0, s, m, static_cast<const uint32_t*>(nullptr), d[0], d[1],
                     d[2], R.inv, R.range, vox, st);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (hs.bad & kClusterBadFinite) return fail(FDM_ERR_INVALID, "a coordinate is not finite (undefined in the reference)");
  if (hs.bad & kClusterBadVoxel)
    return fail(FDM_ERR_INVALID, "a voxel coordinate is outside -2^20 + range .. 2^20 - 1 - range (clamped in the reference)");
  ClusterBox B;
  unsigned key_bits = 0;
  if (!cluster::box(hs.lo, hs.hi, R.range, B, key_bits)) return fail(FDM_ERR_HIP, "the voxels' bounding box is empty");
  g_ror_stats.key_bits = key_bits;
  HIPCK(mark(1));
  // 2. keys over the box, the stable sort, the points in sorted order (its step 2)
  hipLaunchKernelGGL(k_cluster_keys, dim3(blocks), dim3(256), 0, s, m, vox, B, S.pairs.keys[0]);
  const int side = rs_enqueue(s, S.pairs, m, key_bits);
  hipLaunchKernelGGL(k_cluster_gather, dim3(blocks), dim3(256), 0, s, m, S.pairs.idx[side],
                     static_cast<const uint32_t*>(nullptr), d[0], d[1], d[2], pts);
  HIPCK(hipGetLastError());
  HIPCK(mark(2));
  // 3. the candidate tests of the full neighbourhood, and the work bound.  k_ror_count's rate in count mode, measured on
  // the MI355X (profiles/r20/filters/README.md), is written beside filter::kMaxTests' definition.
  const unsigned long long* const keys = S.pairs.keys[side];
  hipLaunchKernelGGL(k_ror_stat_init, dim3(1), dim3(64), 0, s, rst);
  hipLaunchKernelGGL(k_ror_candidates, dim3(blocks), dim3(256), 0, s, m, keys, B, rst);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(&hr, rst, sizeof(hr), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  g_ror_stats.candidate_tests = hr.candidates;
  if (hr.candidates > filter::kMaxTests)
    return fail(FDM_ERR_INVALID, "more than 1.5e11 candidate tests: the voxels are too dense for this radius "
                                 "(refused instead of running for a second or more)");
  HIPCK(mark(3));
  // 4. the counts (from here on the outputs are written)
  uint8_t* d_keep = keep;
  uint32_t* d_counts = counts;
  if (host) {
    const size_t cap = cloud_stride(m);
    if (int rc = b_out.alloc(cap * sizeof(uint32_t) + cap)) return rc;
    d_counts = counts ? b_out.as<uint32_t>() : nullptr;
    d_keep = b_out.as<uint8_t>() + cap * sizeof(uint32_t);
  }
  const uint32_t limit = min_neighbors > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(min_neighbors);
  hipLaunchKernelGGL(k_ror_count, dim3(blocks), dim3(256), 0, s, m, keys, B, pts, R.r_sq, limit, d_keep, d_counts, rst);
  HIPCK(hipGetLastError());
  HIPCK(mark(4));
  if (host) {
    HIPCK(hipMemcpyAsync(keep, d_keep, size_t(m), hipMemcpyDeviceToHost, s));
    if (counts) HIPCK(hipMemcpyAsync(counts, d_counts, size_t(m) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  HIPCK(hipMemcpyAsync(&hr, rst, sizeof(hr), hipMemcpyDeviceToHost, s));
  HIPCK(mark(5));
  HIPCK(hipStreamSynchronize(s));
  if (hr.tests > hr.candidates || (counts && hr.tests != hr.candidates))
    return fail(FDM_ERR_HIP, "the distance tests made do not add up to the candidate tests");
  g_ror_stats.tests_done = hr.tests;
  g_ror_stats.n_kept = hr.kept;
  for (int q = 0; q < 5 && clock; ++q) g_ror_stats.ms[q] = E.ms(q, q + 1);
  *n_kept = hr.kept;
  return FDM_OK;
}

int fdm_cloud_crop(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                   const fdm_crop_config* cfg, int device, uint8_t* keep, uint64_t* n_kept) {
  if (!n_kept) return fail(FDM_ERR_INVALID, "null argument");
  *n_kept = 0;
  if (!cfg) return fail(FDM_ERR_INVALID, "null argument");
  if (n >= (1ull << 32)) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-1");
  if (n && (!x || !y || !z)) return fail(FDM_ERR_INVALID, "null coordinate array");
  if (n && !keep) return fail(FDM_ERR_INVALID, "null argument");
  filter::KeepParams P;
  if (!filter::keep_params(cfg->kind, cfg->mode, cfg->lo, cfg->hi, P))
    return fail(FDM_ERR_INVALID, "kind must be FDM_CROP_BOX .. FDM_CROP_FINITE and mode FDM_CROP_INSIDE or FDM_CROP_OUTSIDE");
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  if (n == 0) return FDM_OK;
  hipStream_t s = nullptr;
  const bool host = on_device == 0;
  const unsigned m = unsigned(n), blocks = std::min((m + 255u) / 256u, kFilterMaxBlocks);
  CloudBlock b_in;
  const float* d[3] = {nullptr, nullptr, nullptr};
  const void* const src[3] = {x, y, z};
  if (int rc = stage_cloud(s, n, 3, src, !host, b_in, d)) return rc;
  DevBuf b_kept, b_out;
  if (int rc = b_kept.alloc(sizeof(unsigned long long))) return rc;
  uint8_t* d_keep = keep;
  if (host) {
    if (int rc = b_out.alloc(size_t(m))) return rc;
    d_keep = b_out.as<uint8_t>();
  }
  unsigned long long* const d_kept = b_kept.as<unsigned long long>();
  hipLaunchKernelGGL(k_filter_stat_init, dim3(1), dim3(64), 0, s, d_kept);
  hipLaunchKernelGGL(k_filter_keep, dim3(blocks), dim3(256), 0, s, m, d[0], d[1], d[2], P, d_keep, d_kept);
  HIPCK(hipGetLastError());
  unsigned long long total = 0ull;
  if (host) HIPCK(hipMemcpyAsync(keep, d_keep, size_t(m), hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(&total, d_kept, sizeof(total), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  *n_kept = total;
  return FDM_OK;
}

}  // extern "C"
