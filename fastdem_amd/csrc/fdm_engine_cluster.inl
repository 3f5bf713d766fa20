// fdm_engine_cluster.inl — host side of Euclidean clustering (kernels: fdm_cluster.hpp; the relation's constants, the
// key layouts and the work bound: fdm_cluster_host.hpp): entry points fdm_cloud_cluster and fdm_cluster_last_stats.
// Part of fdm_engine_post.hip, behind fdm_engine_cloud.inl (DevBuf, Events, the cloud staging) and
// fdm_engine_segment.inl (SortBufs64, Compactor).  Engine-free like the other cloud calls: a call picks its device, works
// on the null stream in scratch of its own and frees it on return.  Synchronous.  Nothing is written to the caller's
// outputs before the last refusal has been decided.

namespace {
thread_local fdm_cluster_stats g_cluster_stats = {};

fdm_cluster_config cluster_defaults() { return fdm_cluster_config{0.5f, 10u, 100000u}; }

// offsets[0] = 0 where the cloud is: all an empty result holds
int cluster_empty(hipStream_t s, bool host, uint32_t* offsets, uint32_t* labels, unsigned m) {
  if (host) {
    offsets[0] = 0u;
    if (labels && m) std::memset(labels, 0, size_t(m) * sizeof(uint32_t));
    return FDM_OK;
  }
  HIPCK(hipMemsetAsync(offsets, 0, sizeof(uint32_t), s));
  if (labels && m) HIPCK(hipMemsetAsync(labels, 0, size_t(m) * sizeof(uint32_t), s));
  HIPCK(hipStreamSynchronize(s));
  return FDM_OK;
}
}  // namespace

extern "C" {

int fdm_cluster_last_stats(fdm_cluster_stats* out) {
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  *out = g_cluster_stats;
  return FDM_OK;
}

int fdm_cloud_cluster(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                      const uint32_t* indices, uint64_t n_indices, const fdm_cluster_config* cfg, int device,
                      uint32_t* cluster_indices, uint32_t* offsets, uint32_t* labels, uint64_t* n_clusters) {
  g_cluster_stats = fdm_cluster_stats{};
  if (!n_clusters) return fail(FDM_ERR_INVALID, "null argument");
  *n_clusters = 0;
  const fdm_cluster_config K = cfg ? *cfg : cluster_defaults();
  const uint64_t m64 = indices ? n_indices : n;
  if (n >= (1ull << 32)) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-1");
  // (the sorts count their tiles of up to 4 096 pairs, and every kernel here its blocks, in 32 bits)
  if (m64 >= 0xFFFFFFFFull - kRsTile) return fail(FDM_ERR_INVALID, "the list has 2^32-4097 entries or more");
  if (n && (!x || !y || !z)) return fail(FDM_ERR_INVALID, "null coordinate array");
  if (!offsets || (m64 && !cluster_indices)) return fail(FDM_ERR_INVALID, "null argument");
  cluster::Relation R;
  if (!cluster::relation(K.tolerance, R))
    return fail(FDM_ERR_INVALID, "tolerance must be a positive finite number whose voxel range is 1 or 2");
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  hipStream_t s = nullptr;
  const bool host = on_device == 0;
  const unsigned np = unsigned(n), m = unsigned(m64), blocks = (m + 255u) / 256u;
  g_cluster_stats.n_points = m;
  g_cluster_stats.range = R.range;
  if (m == 0) return cluster_empty(s, host, offsets, labels, 0u);  // (:127-130, :201-205)

  Events E;
  const bool clock = cloud_profile_on();
  if (clock)
    if (int rc = E.init(7)) return rc;
  auto mark = [&](int k) { return clock ? hipEventRecord(E.ev[k], s) : hipSuccess; };

  CloudBlock b_in;
  const float* d[3] = {nullptr, nullptr, nullptr};
  if (np) {
    const void* const src[3] = {x, y, z};
    if (int rc = stage_cloud(s, n, 3, src, !host, b_in, d)) return rc;
  }
  DevBuf b_idx, b_stat, b_seg, b_pts, b_iv, b_uf, b_keep, b_counts, b_out;
  SortBufs64 S;
  const uint32_t* d_idx = indices;
  if (host && indices) {
    if (int rc = b_idx.alloc(size_t(m) * sizeof(uint32_t))) return rc;
    HIPCK(hipMemcpyAsync(b_idx.p, indices, size_t(m) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    d_idx = b_idx.as<uint32_t>();
  }
  const int rows = cluster_rows(R.range);
  const size_t cap = cloud_stride(m);
  if (int rc = b_stat.alloc(sizeof(ClusterStat))) return rc;
  if (int rc = b_seg.alloc(sizeof(SegStat))) return rc;
  if (int rc = S.alloc(m)) return rc;
  if (int rc = b_pts.alloc(size_t(m) * sizeof(float4))) return rc;
  if (int rc = b_iv.alloc(size_t(2 * rows) * m * sizeof(uint32_t))) return rc;
  if (int rc = b_uf.alloc(3 * cap * sizeof(uint32_t))) return rc;
  if (int rc = b_keep.alloc(size_t(m))) return rc;
  if (int rc = b_counts.alloc((size_t(blocks) + 1) * sizeof(uint32_t))) return rc;
  ClusterStat* const st = b_stat.as<ClusterStat>();
  float4* const pts = b_pts.as<float4>();
  uint32_t* const iv = b_iv.as<uint32_t>();
  uint32_t* const parent = b_uf.as<uint32_t>();
  uint32_t* const size = parent + cap;
  uint32_t* const root = size + cap;
  uint8_t* const keep = b_keep.as<uint8_t>();
  uint32_t* const counts = b_counts.as<uint32_t>();
  ClusterStat hs{};
  auto read_stat = [&]() {
    if (hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s) != hipSuccess) return hipErrorUnknown;
    return hipStreamSynchronize(s);
  };

  // 1. the list alone, then the voxels and what is refused about them
  HIPCK(mark(0));
  if (d_idx) {
    SegStat* const sg = b_seg.as<SegStat>();
    hipLaunchKernelGGL(k_seg_stat_init, dim3(1), dim3(64), 0, s, sg);
    hipLaunchKernelGGL(k_seg_index_check, dim3(std::min(blocks, 2048u)), dim3(256), 0, s, m, d_idx, np, sg);
    HIPCK(hipGetLastError());
    SegStat hg{};
    HIPCK(hipMemcpyAsync(&hg, sg, sizeof(hg), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (hg.bad) return fail(FDM_ERR_INVALID, "an index of the list is not below the point count");
  }
  unsigned long long* const vox = S.pairs.keys[1];  // (the sort's other side: free until its first pass)
  hipLaunchKernelGGL(k_cluster_stat_init, dim3(1), dim3(64), 0, s, st);
  hipLaunchKernelGGL(k_cluster_voxels, dim3(blocks), dim3(256), 0, s, m, d_idx, d[0], d[1], d[2], R.inv, R.range, vox, st);
  HIPCK(hipGetLastError());
  HIPCK(read_stat());
  if (hs.bad & kClusterBadFinite) return fail(FDM_ERR_INVALID, "a coordinate is not finite (undefined in the reference)");
  if (hs.bad & kClusterBadVoxel)
    return fail(FDM_ERR_INVALID, "a voxel coordinate is outside -2^20 + range .. 2^20 - 1 - range (clamped in the reference)");
  ClusterBox B;
  unsigned key_bits = 0;
  if (!cluster::box(hs.lo, hs.hi, R.range, B, key_bits)) return fail(FDM_ERR_HIP, "the voxels' bounding box is empty");
  g_cluster_stats.key_bits = key_bits;
  HIPCK(mark(1));
  // 2. keys over the box, the stable sort, the points in sorted order
  hipLaunchKernelGGL(k_cluster_keys, dim3(blocks), dim3(256), 0, s, m, vox, B, S.pairs.keys[0]);
  const int side = rs_enqueue(s, S.pairs, m, key_bits);
  hipLaunchKernelGGL(k_cluster_gather, dim3(blocks), dim3(256), 0, s, m, S.pairs.idx[side], d_idx, d[0], d[1], d[2], pts);
  HIPCK(hipGetLastError());
  HIPCK(mark(2));
  // 3. the candidate intervals and the work they stand for
  hipLaunchKernelGGL(k_cluster_ranges, dim3(blocks), dim3(256), 0, s, m, S.pairs.keys[side], B, iv, st);
  HIPCK(hipGetLastError());
  HIPCK(read_stat());
  g_cluster_stats.candidate_pairs = hs.pairs;
  if (hs.pairs > cluster::kMaxPairs)
    return fail(FDM_ERR_INVALID, "more than 1.5e11 candidate pairs: the voxels are too dense for this tolerance "
                                 "(refused instead of running for a second or more)");
  HIPCK(mark(3));
  // 4. the components
  hipLaunchKernelGGL(k_cluster_init, dim3(blocks), dim3(256), 0, s, m, parent, size);
  hipLaunchKernelGGL(k_cluster_merge, dim3(blocks), dim3(256), 0, s, m, pts, iv, rows, R.r_sq, parent, st);
  HIPCK(hipGetLastError());
  HIPCK(mark(4));
  // 5. roots, sizes, the kept positions (into the ordering sort's index side)
  hipLaunchKernelGGL(k_cluster_flatten, dim3(blocks), dim3(256), 0, s, m, parent, root, size, st);
  hipLaunchKernelGGL(k_cluster_flags, dim3(blocks), dim3(256), 0, s, m, root, size, K.min_size, K.max_size, keep, st);
  HIPCK(hipGetLastError());
  Compactor pack;
  uint32_t total = 0;
  if (int rc = pack.run(s, m, keep, nullptr, S.pairs.idx[0], &total)) return rc;
  HIPCK(read_stat());
  if (hs.err & kClusterErrFind) return fail(FDM_ERR_HIP, "a find of the union-find did not end within m steps");
  if (hs.err & kClusterErrRetry) return fail(FDM_ERR_HIP, "a unite of the union-find lost its swap more than 4096 times");
  if (hs.unions + hs.components != m || hs.kept > hs.components)
    return fail(FDM_ERR_HIP, "the unions made and the components found do not add up to the list");
  g_cluster_stats.tests = hs.pairs;
  g_cluster_stats.neighbour_pairs = hs.hits;
  g_cluster_stats.unions = hs.unions;
  g_cluster_stats.n_components = hs.components;
  g_cluster_stats.n_kept = hs.kept;
  g_cluster_stats.n_rejected = hs.components - hs.kept;
  g_cluster_stats.n_clustered = total;
  HIPCK(mark(5));
  // 6. the order, offsets, indices, labels
  if (total == 0) {
    if (int rc = cluster_empty(s, host, offsets, labels, m)) return rc;
  } else {
    uint32_t* d_ci = cluster_indices;
    uint32_t* d_off = offsets;
    uint32_t* d_lab = labels;
    if (host) {
      if (int rc = b_out.alloc((3 * cap + 4) * sizeof(uint32_t))) return rc;
      d_ci = b_out.as<uint32_t>();
      d_lab = labels ? d_ci + cap : nullptr;
      d_off = d_ci + 2 * cap;
    }
    unsigned bits_root = 0, order_bits = 0;
    cluster::order_bits(m, bits_root, order_bits);
    const unsigned tblocks = (total + 255u) / 256u;
    hipLaunchKernelGGL(k_cluster_order_keys, dim3(tblocks), dim3(256), 0, s, total, S.pairs.idx[0], root, size, m,
                       bits_root, S.pairs.keys[0]);
    const int oside = rs_enqueue(s, S.pairs, total, order_bits, 0, kRsIdxGiven);
    const unsigned long long* const okeys = S.pairs.keys[oside];
    hipLaunchKernelGGL(k_seg_head_count, dim3(tblocks), dim3(256), 0, s, total, okeys, counts);
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, s, counts, tblocks);
    HIPCK(hipGetLastError());
    uint32_t runs = 0;
    HIPCK(hipMemcpyAsync(&runs, counts + tblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (runs != hs.kept) return fail(FDM_ERR_HIP, "the ordered runs are not the kept components");
    // (from here on the outputs are written)
    hipLaunchKernelGGL(k_seg_heads, dim3(tblocks), dim3(256), 0, s, total, okeys, counts, d_off);
    if (d_lab) HIPCK(hipMemsetAsync(d_lab, 0, size_t(m) * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_cluster_emit, dim3(tblocks), dim3(256), 0, s, total, okeys, counts, S.pairs.idx[oside], d_idx,
                       d_ci, d_lab);
    HIPCK(hipGetLastError());
    if (host) {
      HIPCK(hipMemcpyAsync(cluster_indices, d_ci, size_t(total) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIPCK(hipMemcpyAsync(offsets, d_off, (size_t(runs) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      if (labels) HIPCK(hipMemcpyAsync(labels, d_lab, size_t(m) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
  }
  HIPCK(mark(6));
  HIPCK(hipStreamSynchronize(s));
  for (int q = 0; q < 6 && clock; ++q) g_cluster_stats.ms[q] = E.ms(q, q + 1);
  *n_clusters = hs.kept;
  return FDM_OK;
}

}  // extern "C"
