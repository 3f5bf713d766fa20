// fdm_engine_segment.inl — host side of cloud segmentation (kernels: fdm_segment.hpp; the sampler, the loop's replay and
// the refinement's algebra: fdm_segment_host.hpp): entry points fdm_cloud_segment_ground, fdm_cloud_segment_plane,
// fdm_cloud_segment_planes and fdm_segment_last_stats.  Part of fdm_engine_post.hip, behind fdm_engine_cloud.inl (DevBuf,
// Events, the cloud staging) and fdm_engine_dem.inl (SortBufs).  Engine-free like the other cloud calls: a call picks its device, works on the
// null stream in scratch of its own and frees it on return.  Synchronous: RANSAC reads one PlaneBatch per batch.

namespace {
thread_local fdm_segment_stats g_segment_stats = {};

// SortBufs (fdm_engine_dem.inl) for 64-bit keys: the two sides of a radix sort of n pairs and its histograms
struct SortBufs64 {
  DevBuf mem;
  RsPairs<unsigned long long> pairs{};
  int alloc(unsigned n) {
    const size_t cap = cloud_stride(n);
    if (int rc = mem.alloc(2 * cap * sizeof(unsigned long long) + (2 * cap + rs_hist_words(n)) * sizeof(uint32_t))) return rc;
    unsigned long long* const k = mem.as<unsigned long long>();
    uint32_t* const b = reinterpret_cast<uint32_t*>(k + 2 * cap);
    pairs = {{k, k + cap}, {b, b + cap}, b + 2 * cap};
    return FDM_OK;
  }
};

unsigned seg_bits(uint64_t max_value) {  // bits a value of 0 .. max_value needs, at least one
  unsigned bits = 1;
  while (bits < 64u && (max_value >> bits) != 0u) ++bits;
  return bits;
}

// The flagged positions of a list of m flags, their entries of src (NULL: the positions themselves) written to d_out
// (NULL: counted only) in order; *total = how many.  Synchronises s.
struct Compactor {
  DevBuf b_counts;
  unsigned cap_blocks = 0;
  int ensure(unsigned m) {
    const unsigned blocks = (m + 255u) / 256u;
    if (blocks <= cap_blocks && b_counts.p) return FDM_OK;
    if (b_counts.p) { (void)hipFree(b_counts.p); b_counts.p = nullptr; }
    cap_blocks = blocks;
    return b_counts.alloc((size_t(blocks) + 1) * sizeof(uint32_t));
  }
  int run(hipStream_t s, unsigned m, const uint8_t* d_keep, const uint32_t* src, uint32_t* d_out, uint32_t* total) {
    *total = 0;
    if (m == 0) return FDM_OK;
    if (int rc = ensure(m)) return rc;
    const unsigned blocks = (m + 255u) / 256u;
    uint32_t* const counts = b_counts.as<uint32_t>();
    hipLaunchKernelGGL(k_dem_count, dim3(blocks), dim3(256), 0, s, m, d_keep, counts);
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, s, counts, blocks);
    if (d_out) hipLaunchKernelGGL(k_seg_compact, dim3(blocks), dim3(256), 0, s, m, d_keep, counts, src, d_out);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(total, counts + blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (*total > m) return fail(FDM_ERR_HIP, "a compaction's count overran its list");
    return FDM_OK;
  }
};

fdm_ground_seg_config ground_defaults() { return fdm_ground_seg_config{0.5f, 0.2f, 0.3f, 0.5f, 2u}; }
fdm_ransac_config ransac_defaults() { return fdm_ransac_config{0.1f, 1000, 0.99, 3u, 1}; }
fdm_ransac_result ransac_empty() {  // RansacResult{} (ransac_plane.hpp:42, :80-81)
  fdm_ransac_result r{};
  r.coefficients[2] = 1.0f;
  return r;
}

// iterations per scoring launch.  Measured at 32 / 64 / 128 (profiles/r12/segment/README.md): a loop of 300 - 500 passes
// takes 0.48 / 0.35 / 0.28 ms at 28.8 K points and 1.08 / 0.79 / 0.53 ms at 2.1 M; one that ends after 3 passes pays
// 0.180 / 0.187 / 0.194 ms at 272 K for the hypotheses it did not need
constexpr int kSegBatch = 128;
static_assert(kSegBatch <= kSegMaxBatch, "a PlaneBatch holds the batch");
thread_local int g_segment_batch = kSegBatch;  // fdm_segment_debug_batch

void launch_plane_count(hipStream_t s, unsigned m, const uint32_t* idx, const float* const* c, float thr, int nb,
                        PlaneBatch* B) {
  const unsigned blocks = std::min((m + kSegTile - 1u) / kSegTile, 2048u);
  hipLaunchKernelGGL(k_plane_count, dim3(blocks), dim3(256), 0, s, m, idx, c[0], c[1], c[2], thr, nb, B);
}

// One segmentPlane over a device cloud and a device index list (NULL: every point), and what it leaves for the caller on
// the device: the flag of every list position (d_keep) and the inlier list (d_inl).
struct PlaneCall {
  hipStream_t s = nullptr;
  unsigned n = 0;                 // points of the cloud
  const float* c[3] = {};         // its device channels
  DevBuf b_batch, b_trip, b_keep, b_partial, b_sums, b_stat;
  Compactor pack;
  Events E;
  bool clock = false;
  int batch = g_segment_batch;
  uint8_t* d_keep = nullptr;

  int prepare(unsigned n_, const float* const* ch, unsigned list_cap) {
    n = n_;
    for (int k = 0; k < 3; ++k) c[k] = ch[k];
    clock = cloud_profile_on();
    if (clock)
      if (int rc = E.init(2)) return rc;
    if (int rc = b_batch.alloc(sizeof(PlaneBatch))) return rc;
    if (int rc = b_trip.alloc(size_t(3) * kSegMaxBatch * sizeof(uint32_t))) return rc;
    if (int rc = b_keep.alloc(size_t(list_cap))) return rc;
    if (int rc = b_partial.alloc(size_t(kSegSumBlocks) * 6 * sizeof(double))) return rc;
    if (int rc = b_sums.alloc(6 * sizeof(double))) return rc;
    if (int rc = b_stat.alloc(sizeof(SegStat))) return rc;
    d_keep = b_keep.as<uint8_t>();
    return pack.ensure(list_cap);
  }
  int tick() {
    if (clock) HIPCK(hipEventRecord(E.ev[0], s));
    return FDM_OK;
  }
  int tock(int slot) {  // (the stream is idle by the time the interval is read)
    if (!clock) return FDM_OK;
    HIPCK(hipEventRecord(E.ev[1], s));
    HIPCK(hipEventSynchronize(E.ev[1]));
    g_segment_stats.ms[slot] += E.ms(0, 1);
    return FDM_OK;
  }
  // an index >= n, by a pass that reads the list alone
  int check_indices(const uint32_t* d_idx, unsigned m) {
    if (!d_idx || m == 0) return FDM_OK;
    SegStat* const st = b_stat.as<SegStat>();
    hipLaunchKernelGGL(k_seg_stat_init, dim3(1), dim3(64), 0, s, st);
    hipLaunchKernelGGL(k_seg_index_check, dim3(std::min((m + 255u) / 256u, 2048u)), dim3(256), 0, s, m, d_idx, n, st);
    HIPCK(hipGetLastError());
    SegStat hs{};
    HIPCK(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (hs.bad) return fail(FDM_ERR_INVALID, "an index of the list is not below the point count");
    return FDM_OK;
  }
  // collectInliers (:102-121) with `model`: d_keep, and the list in d_inl (capacity m)
  int collect(const uint32_t* d_idx, unsigned m, const float model[4], float thr, uint32_t* d_inl, uint32_t* total) {
    hipLaunchKernelGGL(k_plane_flags, dim3((m + 255u) / 256u), dim3(256), 0, s, m, d_idx, c[0], c[1], c[2],
                       make_float4(model[0], model[1], model[2], model[3]), thr, d_keep);
    return pack.run(s, m, d_keep, d_idx, d_inl, total);
  }
  // refinePlane (:134-188) over `count` >= 3 listed inliers; best: the unrefined model, for the sign
  int refine(const uint32_t* d_inl, unsigned count, const float best[4], float out[4]) {
    const unsigned blocks = seg_sum_blocks(count);
    double* const part = b_partial.as<double>();
    double* const sums = b_sums.as<double>();
    double h[6];
    hipLaunchKernelGGL(k_plane_sum<false>, dim3(blocks), dim3(256), 0, s, count, d_inl, c[0], c[1], c[2], 0.0, 0.0, 0.0, part);
    hipLaunchKernelGGL(k_plane_sum_final<3>, dim3(1), dim3(256), 0, s, blocks, part, sums);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(h, sums, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    const double centroid[3] = {h[0] / double(count), h[1] / double(count), h[2] / double(count)};  // :148
    hipLaunchKernelGGL(k_plane_sum<true>, dim3(blocks), dim3(256), 0, s, count, d_inl, c[0], c[1], c[2], centroid[0],
                       centroid[1], centroid[2], part);
    hipLaunchKernelGGL(k_plane_sum_final<6>, dim3(1), dim3(256), 0, s, blocks, part, sums);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(h, sums, 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    double v[3];
    seg::smallest_eigenvector(h, v);
    seg::refined_model(v, centroid, best, out);
    return FDM_OK;
  }
  // segmentPlane (:241-334) over m list entries; d_inl: capacity m.  The list has been checked.
  int run(const uint32_t* d_idx, unsigned m, const fdm_ransac_config& cfg, uint32_t* d_inl, fdm_ransac_result* R) {
    *R = ransac_empty();
    if (m < 3) return FDM_OK;  // :247
    seg::XorShift64 rng(42);   // :251
    seg::Loop loop;
    loop.start(m, cfg.max_iterations, cfg.probability);
    float best[4] = {0.0f, 0.0f, 1.0f, 0.0f};  // PlaneModel{}
    PlaneBatch* const B = b_batch.as<PlaneBatch>();
    uint32_t* const d_trip = b_trip.as<uint32_t>();
    PlaneBatch hb;
    uint32_t trip[3 * kSegMaxBatch];
    g_segment_stats.batch = uint32_t(batch);
    if (int rc = tick()) return rc;
    while (loop.running()) {
      const int nb = std::min(batch, loop.remaining());
      for (int j = 0; j < nb; ++j) seg::draw_triplet(rng, m, trip + 3 * j);
      HIPCK(hipMemcpyAsync(d_trip, trip, size_t(3) * nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_plane_models, dim3(1), dim3(kSegMaxBatch), 0, s, nb, d_trip, d_idx, c[0], c[1], c[2], B);
      launch_plane_count(s, m, d_idx, c, cfg.distance_threshold, nb, B);
      HIPCK(hipGetLastError());
      HIPCK(hipMemcpyAsync(&hb, B, sizeof(hb), hipMemcpyDeviceToHost, s));
      HIPCK(hipStreamSynchronize(s));  // (also: `trip` may be rewritten)
      g_segment_stats.n_batches += 1;
      g_segment_stats.n_hypotheses += uint64_t(nb);
      for (int j = 0; j < nb; ++j)
        if (hb.count[j] > m) return fail(FDM_ERR_HIP, "an inlier count overran its list");
      const int upd = loop.replay(hb.count, hb.valid, nb);
      if (upd >= 0) { best[0] = hb.model[upd].x; best[1] = hb.model[upd].y; best[2] = hb.model[upd].z; best[3] = hb.model[upd].w; }
    }
    g_segment_stats.n_invalid_samples += loop.n_invalid;
    if (int rc = tock(0)) return rc;
    if (loop.best_count < cfg.min_inliers) return FDM_OK;  // :310
    if (int rc = tick()) return rc;
    uint32_t total = 0;
    if (int rc = collect(d_idx, m, best, cfg.distance_threshold, d_inl, &total)) return rc;
    if (int rc = tock(1)) return rc;
    float model[4] = {best[0], best[1], best[2], best[3]};
    if (cfg.refine_model && total >= 3) {  // :321
      if (int rc = tick()) return rc;
      float refined[4];
      if (int rc = refine(d_inl, total, best, refined)) return rc;
      if (int rc = tock(2)) return rc;
      if (std::isfinite(refined[3])) {     // :323
        std::memcpy(model, refined, sizeof(model));
        if (int rc = tick()) return rc;
        if (int rc = collect(d_idx, m, model, cfg.distance_threshold, d_inl, &total)) return rc;
        if (int rc = tock(1)) return rc;
      }
    }
    std::memcpy(R->coefficients, model, sizeof(model));
    R->n_inliers = total;
    R->fitness = static_cast<double>(total) / double(m);  // :330
    R->iterations = loop.iter;
    R->success = (std::isfinite(model[3]) && total > 0) ? 1 : 0;  // ransac_plane.hpp:92-94
    return FDM_OK;
  }
};

// what the plane entries refuse before a device is touched
int plane_check(uint64_t n, const float* x, const float* y, const float* z, uint64_t n_list, const fdm_ransac_config& cfg) {
  if (n >= (1ull << 32)) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-1");
  // (every kernel over the list counts its blocks of 256 positions in 32 bits, as the sorts do)
  if (n_list > 0xFFFFFFFFull - kRsTile) return fail(FDM_ERR_INVALID, "the index list exceeds 2^32-4097 entries");
  if (n && (!x || !y || !z)) return fail(FDM_ERR_INVALID, "null coordinate array");
  if (cfg.distance_threshold != cfg.distance_threshold) return fail(FDM_ERR_INVALID, "distance_threshold must be a number");
  return FDM_OK;
}
}  // namespace

extern "C" {

int fdm_segment_debug_batch(int batch) {
  if (batch < 0 || batch > kSegMaxBatch) return fail(FDM_ERR_INVALID, "batch must be 0 (the default) or 1 .. 128");
  g_segment_batch = batch ? batch : kSegBatch;
  return FDM_OK;
}

int fdm_segment_last_stats(fdm_segment_stats* out) {
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  *out = g_segment_stats;
  return FDM_OK;
}

int fdm_cloud_segment_ground(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                             const fdm_ground_seg_config* cfg, int device, uint32_t* ground, uint32_t* obstacles,
                             uint64_t* n_ground, uint64_t* n_obstacles) {
  g_segment_stats = fdm_segment_stats{};
  if (!n_ground || !n_obstacles) return fail(FDM_ERR_INVALID, "null argument");
  *n_ground = *n_obstacles = 0;
  const fdm_ground_seg_config G = cfg ? *cfg : ground_defaults();
  if (int rc = check_resolution(G.grid_resolution)) return rc;
  if (!(G.cell_percentile >= 0.0f)) return fail(FDM_ERR_INVALID, "cell_percentile must not be negative or NaN");
  // (the sorts count their tiles of up to 4 096 pairs, and every kernel here its blocks, in 32 bits: n + 4 096 must fit)
  if (n > 0xFFFFFFFFull - kRsTile) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-4097");
  if (n == 0) return FDM_OK;  // :72-74
  if (!x || !y || !z) return fail(FDM_ERR_INVALID, "null coordinate array");
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  hipStream_t s = nullptr;
  const unsigned np = unsigned(n), blocks = (np + 255u) / 256u;
  const bool host = on_device == 0;
  Events E;
  const bool clock = cloud_profile_on();
  if (clock)
    if (int rc = E.init(5)) return rc;
  auto mark = [&](int k) { return clock ? hipEventRecord(E.ev[k], s) : hipSuccess; };

  CloudBlock b_in;
  const void* const src[3] = {x, y, z};
  const float* d[3];
  if (int rc = stage_cloud(s, n, 3, src, !host, b_in, d)) return rc;
  DevBuf b_stat, b_cell, b_counts, b_pos, b_cut, b_flags, b_out;
  SortBufs S1;
  SortBufs64 S2;
  if (int rc = b_stat.alloc(sizeof(SegStat))) return rc;
  if (int rc = b_cell.alloc(size_t(np) * sizeof(unsigned long long))) return rc;
  if (int rc = b_counts.alloc((size_t(blocks) + 1) * sizeof(uint32_t))) return rc;
  if (int rc = b_pos.alloc((size_t(np) + 1) * sizeof(uint32_t))) return rc;
  if (int rc = b_cut.alloc(size_t(np) * sizeof(uint32_t))) return rc;
  if (int rc = b_flags.alloc(2 * cloud_stride(np))) return rc;
  if (int rc = S1.alloc(np)) return rc;
  if (int rc = S2.alloc(np)) return rc;
  SegStat* const st = b_stat.as<SegStat>();
  unsigned long long* const cell = b_cell.as<unsigned long long>();
  uint32_t* const counts = b_counts.as<uint32_t>();
  uint32_t* const pos = b_pos.as<uint32_t>();
  uint32_t* const cut = b_cut.as<uint32_t>();
  uint8_t* const is_ground = b_flags.as<uint8_t>();
  uint8_t* const is_obstacle = is_ground + cloud_stride(np);

  // 1. cells, ord(z), the refusal of what the reference leaves undefined
  HIPCK(mark(0));
  hipLaunchKernelGGL(k_seg_stat_init, dim3(1), dim3(64), 0, s, st);
  hipLaunchKernelGGL(k_seg_cell_keys, dim3(blocks), dim3(256), 0, s, np, d[0], d[1], d[2], G.grid_resolution, cell,
                     S1.pairs.keys[0], st);
  HIPCK(hipGetLastError());
  SegStat hs{};
  HIPCK(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (hs.bad)
    return fail(FDM_ERR_INVALID, "a coordinate is not finite, or its cell does not fit an int32 (undefined in the reference)");
  if (hs.min_x > hs.max_x || hs.min_y > hs.max_y) return fail(FDM_ERR_HIP, "the cells' bounding box is empty");
  HIPCK(mark(1));
  // 2. by z, then (stable) by cell: every cell one run, its z ascending
  const int side1 = rs_enqueue(s, S1.pairs, np, 32u);
  const unsigned bits_x = seg_bits(uint64_t(hs.max_x - hs.min_x)), bits_y = seg_bits(uint64_t(hs.max_y - hs.min_y));
  hipLaunchKernelGGL(k_seg_pack_keys, dim3(blocks), dim3(256), 0, s, np, S1.pairs.idx[side1], cell, hs.min_x, hs.min_y,
                     bits_x, S2.pairs.keys[0]);
  HIPCK(hipMemcpyAsync(S2.pairs.idx[0], S1.pairs.idx[side1], size_t(np) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  const int side2 = rs_enqueue(s, S2.pairs, np, bits_x + bits_y, 0, kRsIdxGiven);
  const unsigned long long* const keys = S2.pairs.keys[side2];
  const uint32_t* const idx = S2.pairs.idx[side2];
  HIPCK(hipGetLastError());
  HIPCK(mark(2));
  // 3. run heads, 4. cuts and classification
  const GroundParams GP{G.cell_percentile, G.ground_thickness, G.max_ground_height, G.min_points_per_cell};
  hipLaunchKernelGGL(k_seg_head_count, dim3(blocks), dim3(256), 0, s, np, keys, counts);
  hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, s, counts, blocks);
  hipLaunchKernelGGL(k_seg_heads, dim3(blocks), dim3(256), 0, s, np, keys, counts, pos);
  hipLaunchKernelGGL(k_seg_cell_cut, dim3(blocks), dim3(256), 0, s, np, counts, blocks, pos, idx, d[2], GP, cut);
  hipLaunchKernelGGL(k_seg_classify, dim3(blocks), dim3(256), 0, s, np, keys, idx, counts, cut, d[2], is_ground,
                     is_obstacle);
  HIPCK(hipGetLastError());
  HIPCK(mark(3));
  // 5. the two lists in input order
  uint32_t* d_ground = ground;
  uint32_t* d_obst = obstacles;
  if (host) {
    if (int rc = b_out.alloc(2 * cloud_stride(np) * sizeof(uint32_t))) return rc;
    d_ground = ground ? b_out.as<uint32_t>() : nullptr;
    d_obst = obstacles ? b_out.as<uint32_t>() + cloud_stride(np) : nullptr;
  }
  Compactor pack;
  uint32_t ng = 0, no = 0;
  if (int rc = pack.run(s, np, is_ground, nullptr, d_ground, &ng)) return rc;
  if (int rc = pack.run(s, np, is_obstacle, nullptr, d_obst, &no)) return rc;
  HIPCK(mark(4));
  if (uint64_t(ng) + uint64_t(no) != n) return fail(FDM_ERR_HIP, "the two lists do not hold every point once");
  if (host) {
    if (ground && ng) HIPCK(hipMemcpyAsync(ground, d_ground, size_t(ng) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (obstacles && no) HIPCK(hipMemcpyAsync(obstacles, d_obst, size_t(no) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  HIPCK(hipStreamSynchronize(s));
  for (int q = 0; q < 4 && clock; ++q) g_segment_stats.ms[q] = E.ms(q, q + 1);
  *n_ground = ng;
  *n_obstacles = no;
  return FDM_OK;
}

int fdm_cloud_segment_plane(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                            const uint32_t* indices, uint64_t n_indices, const fdm_ransac_config* cfg, int device,
                            uint32_t* inliers, fdm_ransac_result* result) {
  g_segment_stats = fdm_segment_stats{};
  if (!result) return fail(FDM_ERR_INVALID, "null argument");
  *result = ransac_empty();
  const fdm_ransac_config C = cfg ? *cfg : ransac_defaults();
  const uint64_t m64 = indices ? n_indices : n;
  if (int rc = plane_check(n, x, y, z, m64, C)) return rc;
  if (m64 && !inliers) return fail(FDM_ERR_INVALID, "null argument");
  const unsigned np = unsigned(n), m = unsigned(m64);
  if (m == 0) return FDM_OK;
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  const bool host = on_device == 0;
  PlaneCall call;
  CloudBlock b_in;
  DevBuf b_idx, b_inl;
  const float* d[3] = {nullptr, nullptr, nullptr};
  if (np) {
    const void* const src[3] = {x, y, z};
    if (int rc = stage_cloud(call.s, n, 3, src, !host, b_in, d)) return rc;
  }
  const uint32_t* d_idx = indices;
  uint32_t* d_inl = inliers;
  if (host) {
    if (indices) {
      if (int rc = b_idx.alloc(size_t(m) * sizeof(uint32_t))) return rc;
      HIPCK(hipMemcpyAsync(b_idx.p, indices, size_t(m) * sizeof(uint32_t), hipMemcpyHostToDevice, call.s));
      d_idx = b_idx.as<uint32_t>();
    }
    if (int rc = b_inl.alloc(size_t(m) * sizeof(uint32_t))) return rc;
    d_inl = b_inl.as<uint32_t>();
  }
  if (int rc = call.prepare(np, d, m)) return rc;
  if (int rc = call.check_indices(d_idx, m)) return rc;
  if (int rc = call.run(d_idx, m, C, d_inl, result)) return rc;
  if (host && result->n_inliers)
    HIPCK(hipMemcpyAsync(inliers, d_inl, size_t(result->n_inliers) * sizeof(uint32_t), hipMemcpyDeviceToHost, call.s));
  HIPCK(hipStreamSynchronize(call.s));
  return FDM_OK;
}

int fdm_cloud_segment_planes(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                             const fdm_ransac_config* cfg, uint64_t max_planes, double min_fitness, int device,
                             uint32_t* inliers, fdm_ransac_result* results, uint64_t* n_planes) {
  g_segment_stats = fdm_segment_stats{};
  if (!n_planes) return fail(FDM_ERR_INVALID, "null argument");
  *n_planes = 0;
  const fdm_ransac_config C = cfg ? *cfg : ransac_defaults();
  if (int rc = plane_check(n, x, y, z, n, C)) return rc;
  if (n < 3 || max_planes == 0) return FDM_OK;  // :378
  if (!inliers || !results) return fail(FDM_ERR_INVALID, "null argument");
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  const bool host = on_device == 0;
  const unsigned np = unsigned(n);
  PlaneCall call;
  CloudBlock b_in;
  DevBuf b_rem, b_inl, b_drop;
  const void* const src[3] = {x, y, z};
  const float* d[3];
  if (int rc = stage_cloud(call.s, n, 3, src, !host, b_in, d)) return rc;
  if (int rc = b_rem.alloc(2 * cloud_stride(np) * sizeof(uint32_t))) return rc;  // the remaining indices, two sides
  if (int rc = b_drop.alloc(size_t(np))) return rc;
  uint32_t* d_out = inliers;
  if (host) {
    if (int rc = b_inl.alloc(size_t(np) * sizeof(uint32_t))) return rc;
    d_out = b_inl.as<uint32_t>();
  }
  if (int rc = call.prepare(np, d, np)) return rc;
  uint32_t* rem[2] = {b_rem.as<uint32_t>(), b_rem.as<uint32_t>() + cloud_stride(np)};
  const uint32_t* d_idx = nullptr;  // every point, in order (:373-376)
  unsigned m = np;
  uint64_t taken = 0, planes = 0;
  int side = 0;
  while (planes < max_planes && m >= 3) {  // :378
    fdm_ransac_result R;
    if (int rc = call.run(d_idx, m, C, d_out + taken, &R)) return rc;
    if (!R.success || R.fitness < min_fitness) break;  // :382-384
    // the inliers leave the list, the rest keep their order (:387-399): the flags of the last collect, by position
    if (int rc = call.tick()) return rc;
    uint32_t left = 0;
    hipLaunchKernelGGL(k_seg_invert, dim3((m + 255u) / 256u), dim3(256), 0, call.s, m, call.d_keep, b_drop.as<uint8_t>());
    if (int rc = call.pack.run(call.s, m, b_drop.as<uint8_t>(), d_idx, rem[side], &left)) return rc;
    if (int rc = call.tock(3)) return rc;
    if (uint64_t(left) + R.n_inliers != m) return fail(FDM_ERR_HIP, "the strike-out lost or gained an index");
    d_idx = rem[side];
    side ^= 1;
    m = left;
    taken += R.n_inliers;
    results[planes++] = R;
  }
  if (host && taken) HIPCK(hipMemcpyAsync(inliers, d_out, size_t(taken) * sizeof(uint32_t), hipMemcpyDeviceToHost, call.s));
  HIPCK(hipStreamSynchronize(call.s));
  *n_planes = planes;
  return FDM_OK;
}

}  // extern "C"
