// fdm_engine_ray.inl — host side of the raycasting stage (kernels: fdm_raycast.hpp): voxel sort, ray
// queue, walk, resolve; entry points fdm_engine_apply_raycasting*, fdm_engine_voxel_any, fdm_engine_last_ray_ms.
// The body of fdm_engine_ray.hip (one of the library's five translation units, fdm_engine_host.hpp).
// A stage works in a RayBank (fdm_engine_host.hpp: its buffers, and who may use which bank when) and launches on one
// stream; both are ARGUMENTS of every helper here (RayLane), never state of the engine.  ensure_* allocate, grow and
// initialise a bank on the MAIN stream and may drain every stream (sync_all); enqueue_* only launch, on the lane's
// stream: every ensure_* a stage needs comes before its first enqueue_*.

namespace fdmh {

// ---- raycasting stage (fdm_raycast.hpp) ----
bool voxel_size_ok(float v) { return v >= 0.001f && v <= 100.0f; }  // voxel_grid_impl.hpp:31-33

// raycasting.cpp:223-226: created on first use; invisible until a frame passed the preconditions
int ensure_ray_layers(fdm_engine* e) {
  int rc;
  for (const char* n : {"ghost_removal", "raycasting", "_visibility_logodds"})
    if (!find_layer(e, n) && (rc = add_layer(e, n, NAN, true))) return rc;
  return FDM_OK;
}

// where a stage's launches go: the bank they work in, the stream they are put on
struct RayLane {
  RayBank& b;
  hipStream_t s;
};

// ---- a bank's buffers (ensure_*: on the MAIN stream, whichever stream the stage then takes) ----
int ensure_ray_cells(fdm_engine* e, RayBank& b) {
  if (b.rc_cnt) return FDM_OK;
  HIPCK(hipMalloc(reinterpret_cast<void**>(&b.rc_cnt), e->ncell * sizeof(uint32_t)));
  HIPCK(hipMalloc(reinterpret_cast<void**>(&b.rc_min), e->ncell * sizeof(uint32_t)));
  const int blocks = int(std::min<size_t>((e->ncell + 255) / 256, 4096));
  hipLaunchKernelGGL(k_fill_u32, dim3(blocks), dim3(256), 0, e->stream, b.rc_cnt, 0u, e->ncell);
  hipLaunchKernelGGL(k_fill_u32, dim3(blocks), dim3(256), 0, e->stream, b.rc_min, kRayEmpty, e->ncell);
  // bucket counts (kept at zero between scans by k_ray_bin_scan) | bucket offsets | per-block sums
  const size_t bin_words = 2u * size_t(kRayBins) + kRayBins / kRayBinBlock;
  HIPCK(hipMalloc(reinterpret_cast<void**>(&b.ray_bins), bin_words * sizeof(uint32_t)));
  HIPCK(hipMemsetAsync(b.ray_bins, 0, bin_words * sizeof(uint32_t), e->stream));
  HIPCK(hipGetLastError());
  return FDM_OK;
}

// A bank's voxel / queue buffers for n points with a quarter and 1 024 of slack: what it held is freed first, so nothing of
// the bank may be in flight.  Engine-free: the cloud filters (fdm_engine_voxel.inl) fill a bank of their own with it.
int alloc_voxel_buffers(RayBank& b, size_t n) {
  for (int k = 0; k < 2; ++k) {
    if (b.vkeys[k]) HIPCK(hipFree(b.vkeys[k]));
    if (b.vidx[k]) HIPCK(hipFree(b.vidx[k]));
    b.vkeys[k] = nullptr;
    b.vidx[k] = nullptr;
  }
  if (b.vsel) HIPCK(hipFree(b.vsel));
  if (b.ray_blk) HIPCK(hipFree(b.ray_blk));
  if (b.sort_tmp) HIPCK(hipFree(b.sort_tmp));
  b.vsel = b.ray_blk = b.sort_tmp = nullptr;
  b.vcap = 0;
  const size_t cap = n + n / 4 + 1024;
  for (int k = 0; k < 2; ++k) {
    HIPCK(hipMalloc(reinterpret_cast<void**>(&b.vkeys[k]), cap * sizeof(unsigned long long)));
    HIPCK(hipMalloc(reinterpret_cast<void**>(&b.vidx[k]), cap * sizeof(uint32_t)));
  }
  HIPCK(hipMalloc(reinterpret_cast<void**>(&b.vsel), cap * sizeof(uint32_t)));
  HIPCK(hipMalloc(reinterpret_cast<void**>(&b.ray_blk), (cap / 512u + 2u) * sizeof(uint32_t)));  // (blocks of >= 512 points)
  HIPCK(hipMalloc(reinterpret_cast<void**>(&b.sort_tmp), rs_hist_words(cap) * sizeof(uint32_t)));
  b.vcap = cap;
  return FDM_OK;
}
// (sync_all flushes a held-back stage, which runs in bank 0 and may grow it first: everything is idle afterwards)
int ensure_voxel_buffers(fdm_engine* e, RayBank& b, size_t n) {
  if (n <= b.vcap) return FDM_OK;
  if (int rc_sync = sync_all(e)) return rc_sync;
  return alloc_voxel_buffers(b, n);
}

// Stable sort of the n pairs in (vkeys[src], vidx[src]) by the low `bits` bits of the key; the result lands in
// (vkeys[1], vidx[1]).  `src` must be voxel_sort_source(bits): the buffers alternate once per pass.
int voxel_sort_source(unsigned bits) { return (rs_passes(bits) & 1) ? 0 : 1; }
template <typename KEY>
int enqueue_radix_sort(const RayLane& lane, unsigned n, unsigned bits) {
  const RayBank& b = lane.b;
  const RsPairs<KEY> pairs{{reinterpret_cast<KEY*>(b.vkeys[0]), reinterpret_cast<KEY*>(b.vkeys[1])},
                           {b.vidx[0], b.vidx[1]}, b.sort_tmp};
  // (the first pass's histogram is k_voxel_keys' and its indices are the positions)
  (void)rs_enqueue<KEY>(lane.s, pairs, n, bits, voxel_sort_source(bits), kRsHistGiven);
  HIPCK(hipGetLastError());
  return FDM_OK;
}
// the keys of the scan's points into vkeys[src] (+ the sort's first histogram)
template <typename KEY>
void launch_voxel_keys(fdm_engine* e, const RayLane& lane, unsigned n, float inv, int flag_slot, const VoxelCompact& C,
                       const float* dx, const float* dy, const float* dz, int src) {
  const unsigned tile = rs_tile(n), tiles = (n + tile - 1u) / tile;
  uint32_t* const hist = lane.b.sort_tmp;
  KEY* const keys = reinterpret_cast<KEY*>(lane.b.vkeys[src]);
  if (tile == kRsTileSmall)
    hipLaunchKernelGGL((k_voxel_keys<KEY, kRsTileSmall>), dim3(tiles), dim3(256), 0, lane.s, n, inv, flag_slot, C,
                       e->d_state, dx, dy, dz, keys, lane.b.vsel, tiles, hist);
  else
    hipLaunchKernelGGL((k_voxel_keys<KEY, kRsTile>), dim3(tiles), dim3(256), 0, lane.s, n, inv, flag_slot, C,
                       e->d_state, dx, dy, dz, keys, lane.b.vsel, tiles, hist);
}

// ---- option "voxel_any_order" = 1: the order libstdc++'s std::sort leaves (fdm_introsort.hpp) ----
// Global level passes for n pairs: until no segment is larger than kIsLds, with room for an unbalanced tree (a median of
// three keeps random, sorted and tie-heavy scans within log2(n / kIsLds) + 2); what is still larger after them takes
// k_is_rest.  The launch count depends on n only: no host round trip.
int is_levels(size_t n) {
  if (n <= kIsLds) return 0;
  int lg = 0;
  while ((size_t(kIsLds) << lg) < n) ++lg;
  return std::min(is_depth_limit(unsigned(n)), 2 * lg + 4);
}
size_t is_cap_big(size_t cap) { return cap / (kIsLds + 1u) + 2u; }
size_t is_cap_fin(size_t cap) { return std::min(cap / 2u + 2u, 2u * size_t(is_levels(cap)) * is_cap_big(cap) + 2u); }
size_t is_cap_tiles(size_t cap) { return cap / kIsTile + is_cap_big(cap) + 2u; }
// carve is_buf (laid out for `cap` pairs) into the kernels' arrays; returns the bytes it takes (base 0: only count)
template <typename KEY>
size_t is_layout(uintptr_t base, size_t cap, IsBufs<KEY>* B) {
  size_t off = 0;
  auto take = [&](auto*& p, size_t count) {
    using T = std::remove_reference_t<decltype(*p)>;
    p = reinterpret_cast<T*>(base + off);
    off += (count * sizeof(T) + 255u) & ~size_t(255);
  };
  const size_t cb = is_cap_big(cap), ct = is_cap_tiles(cap);
  for (int k = 0; k < 2; ++k) { take(B->key[k], cap); take(B->idx[k], cap); }
  take(B->posg, cap); take(B->posr, cap);
  take(B->big[0], cb); take(B->big[1], cb); take(B->rest, cb); take(B->fin, is_cap_fin(cap));
  take(B->piv, cb); take(B->tile0, cb); take(B->tot, 2u * cb);
  take(B->tile_seg, ct); take(B->tile_cnt, ct); take(B->tile_ag, ct); take(B->tile_ar, ct); take(B->tile_og, ct);
  take(B->tile_or, ct);
  take(B->ctl, 1u);
  B->cap_big = unsigned(cb);
  B->cap_fin = unsigned(is_cap_fin(cap));
  B->cap_tiles = unsigned(ct);
  return off;
}
int alloc_introsort_buffers(RayBank& b, size_t n) {  // (engine-free, as alloc_voxel_buffers)
  if (b.is_buf) HIPCK(hipFree(b.is_buf));
  b.is_buf = nullptr;
  b.is_cap = 0;
  const size_t cap = n + n / 4u + 1024u;
  IsBufs<unsigned long long> B{};  // (the 64-bit layout is the larger one)
  HIPCK(hipMalloc(&b.is_buf, is_layout(uintptr_t(0), cap, &B)));
  b.is_cap = cap;
  return FDM_OK;
}
int ensure_introsort_buffers(fdm_engine* e, RayBank& b, size_t n) {
  if (n <= b.is_cap) return FDM_OK;
  if (int rc_sync = sync_all(e)) return rc_sync;
  return alloc_introsort_buffers(b, n);
}
// (key, position) of the n pairs in vkeys[0] (k_voxel_keys' output) -> vkeys[1] / vidx[1] in std::sort's order, the
// dropped points behind the valid ones
template <typename KEY>
int enqueue_introsort(const RayLane& lane, unsigned n) {
  IsBufs<KEY> B{};
  is_layout(reinterpret_cast<uintptr_t>(lane.b.is_buf), lane.b.is_cap, &B);
  B.okey = reinterpret_cast<KEY*>(lane.b.vkeys[1]);
  B.oidx = lane.b.vidx[1];
  const KEY* keys = reinterpret_cast<const KEY*>(lane.b.vkeys[0]);
  const unsigned ct = std::max(1u, (n + kIsTile - 1u) / kIsTile);
  hipLaunchKernelGGL(k_is_ccount<KEY>, dim3(ct), dim3(256), 0, lane.s, n, keys, B);
  hipLaunchKernelGGL(k_is_cscan<KEY>, dim3(1), dim3(256), 0, lane.s, ct, B);
  hipLaunchKernelGGL(k_is_cscatter<KEY>, dim3(ct), dim3(256), 0, lane.s, n, keys, B);
  const int levels = is_levels(n);
  const unsigned tiles = unsigned(std::min<size_t>(is_cap_tiles(n), B.cap_tiles));  // bound of a level's tiles
  for (int lv = 0; lv < levels; ++lv) {
    hipLaunchKernelGGL(k_is_plan<KEY>, dim3(1), dim3(256), 0, lane.s, lv, B);
    hipLaunchKernelGGL(k_is_count<KEY>, dim3(tiles), dim3(256), 0, lane.s, lv, B);
    hipLaunchKernelGGL(k_is_scan<KEY>, dim3(1), dim3(256), 0, lane.s, lv, B);
    hipLaunchKernelGGL(k_is_pos<KEY>, dim3(tiles), dim3(256), 0, lane.s, lv, B);
    hipLaunchKernelGGL(k_is_scatter<KEY>, dim3(tiles), dim3(256), 0, lane.s, lv, int(lv == levels - 1), B);
  }
  const unsigned fin_blocks = std::max(1u, std::min(2048u, n / 64u));
  hipLaunchKernelGGL(k_is_finish<KEY>, dim3(fin_blocks), dim3(64), 0, lane.s, B);
  if (levels > 0) hipLaunchKernelGGL(k_is_rest<KEY>, dim3(64), dim3(64), 0, lane.s, B);
  HIPCK(hipGetLastError());
  return FDM_OK;
}

// The compact voxel key of a scan whose points lie in `box` (see plan_voxel_sort): bits == 0 if the box is unknown
// or too large for it.
VoxelCompact voxel_compact_of(float voxel_size, const double* box) {
  const float inv = 1.0f / voxel_size;  // voxel_grid_impl.hpp:46
  VoxelCompact C{0, 0, 0, 0, 0};
  // (a centre beyond 1e9 voxels would overflow the int corner below: every index of it clamps anyway, full key)
  const auto near = [&](double v) { return std::fabs(v) * double(inv) < 1.0e9; };
  if (box && std::isfinite(box[3]) && box[3] > 0.0 && box[3] * double(inv) < 4.0e6 && near(box[0]) && near(box[1]) &&
      near(box[2])) {
    const double half = box[3] + 2.0 * double(voxel_size);  // 2-cell margin for the float transforms
    const int span = int(std::ceil(2.0 * half * double(inv))) + 4;
    int bits = 1;
    while ((1 << bits) < span) ++bits;
    if (3 * bits <= 62 && bits <= 21) {
      C.bits = C.zbits = bits;
      C.x0 = int(std::floor((box[0] - half) * double(inv))) - 1;
      C.y0 = int(std::floor((box[1] - half) * double(inv))) - 1;
      C.z0 = int(std::floor((box[2] - half) * double(inv))) - 1;
      // box[4..5] (optional): map-frame z interval the crops leave (cropZ slab tilted by T_world_base)
      if (std::isfinite(box[4]) && std::isfinite(box[5]) && box[5] > box[4]) {
        const double zlo = std::max(box[4], box[2] - half) - 2.0 * double(voxel_size);
        const double zhi = std::min(box[5], box[2] + half) + 2.0 * double(voxel_size);
        const int zspan = int(std::ceil((zhi - zlo) * double(inv))) + 4;
        int zb = 1;
        while ((1 << zb) < zspan) ++zb;
        if (zb < bits) {
          C.zbits = zb;
          C.z0 = int(std::floor(zlo * double(inv))) - 1;
        }
      }
      // The reference key clamps every voxel index to [-2^20, 2^20 - 1] (voxel.hpp:28-43): far from the origin (UTM
      // northings: 5.3e6 m / 0.2 m = 2.7e7) all points of a scan collapse onto a few clamped voxels.  The rebased key
      // does not clamp, so it is only the same key when no index of the box reaches the clamp; otherwise the full key.
      constexpr long long kMin = -(1ll << 20), kMax = (1ll << 20) - 1;
      const auto inside = [&](int lo, int b) { return lo >= kMin && (long long)lo + (1ll << b) - 1 <= kMax; };
      if (!inside(C.x0, C.bits) || !inside(C.y0, C.bits) || !inside(C.z0, C.zbits)) C = VoxelCompact{0, 0, 0, 0, 0};
    }
  }
  return C;
}

// The box an integrate() scan's preprocessed points lie in: cropRange keeps d^2 <= range_max^2 around the BASE origin,
// i.e. around T_world_base's translation, and cropZ keeps z_base in [z_min, z_max]: z_map = R20 x + R21 y + R22 z + t_z
// with |R20 x + R21 y| <= hypot(R20, R21) * range_max (column-major Twb: R2j = Twb[4 j + 2])
void ray_box_of(const fdm_engine* e, const ScanParams& P, double box[6]) {
  double zlo = NAN, zhi = NAN;
  if (std::isfinite(double(e->cfg.z_min)) && std::isfinite(double(e->cfg.z_max)) &&
      std::fabs(double(e->cfg.z_min)) < 1e6 && std::fabs(double(e->cfg.z_max)) < 1e6 &&
      std::isfinite(double(e->cfg.range_max)) && double(e->cfg.range_max) < 1e6) {
    const double r20 = double(P.Twb[2]), r21 = double(P.Twb[6]), r22 = double(P.Twb[10]);
    const double tilt = std::hypot(r20, r21) * double(e->cfg.range_max);
    const double a = r22 * double(e->cfg.z_min), b = r22 * double(e->cfg.z_max);
    zlo = P.base_z + std::min(a, b) - tilt;
    zhi = P.base_z + std::max(a, b) + tilt;
  }
  box[0] = P.base_x; box[1] = P.base_y; box[2] = P.base_z; box[3] = double(e->cfg.range_max); box[4] = zlo; box[5] = zhi;
}

// How a scan's voxel filter runs, decided once per stage: ensure_voxel_sort and enqueue_voxel_sort both follow it.
// `box` (nullable): centre (3) + half extent [m] of a box that holds every finite point of the cloud, then the
// map-frame z interval [lo, hi] they lie in (NaN, NaN if unknown); with it the compact 32-bit key is used when
// 3 * bits <= 31.  key_mode tells what the bank's buffers hold afterwards: 0 = sorted uint64 keys, 1 = sorted uint32
// compact keys, 2 = points grouped by key bucket, unsorted (the sort-free filter of small scans, k_vs_*).
struct VoxelPlan {
  VoxelCompact C;
  int key_bits;
  int key_mode;
};
VoxelPlan plan_voxel_sort(const fdm_engine* e, unsigned n, float voxel_size, const double* box) {
  VoxelPlan p;
  p.C = voxel_compact_of(voxel_size, box);
  p.key_bits = 2 * p.C.bits + p.C.zbits;
  p.key_mode = (p.C.bits > 0 && p.key_bits <= 31) ? 1 : 0;
  if (p.key_mode == 1 && !e->opt.voxel_any_order && e->opt.voxel_small && n <= unsigned(e->opt.voxel_small_max))
    p.key_mode = 2;
  return p;
}

// what enqueue_voxel_sort(plan) of n points works in
int ensure_voxel_sort(fdm_engine* e, RayBank& b, unsigned n, const VoxelPlan& plan) {
  if (int rc = ensure_voxel_buffers(e, b, n)) return rc;
  if (e->opt.voxel_any_order) return ensure_introsort_buffers(e, b, n);
  if (plan.key_mode != 2) return FDM_OK;
  if (!e->vs_cnt) {
    const size_t words = (size_t(1) << kVsFineBits) + kVsCoarse + 1u;
    HIPCK(hipMalloc(reinterpret_cast<void**>(&e->vs_cnt), words * sizeof(uint32_t)));
    HIPCK(hipMemsetAsync(e->vs_cnt, 0, words * sizeof(uint32_t), e->stream));
  }
  if (e->vs_rec_cap < n) {
    if (int rc_sync = sync_all(e)) return rc_sync;
    if (e->vs_rec) HIPCK(hipFree(e->vs_rec));
    e->vs_rec = nullptr;
    e->vs_rec_cap = std::max<size_t>(size_t(1) << 16, size_t(n) + n / 4);
    HIPCK(hipMalloc(reinterpret_cast<void**>(&e->vs_rec), e->vs_rec_cap * sizeof(uint4)));
  }
  return FDM_OK;
}

// keys -> sort: vkeys[1] / vidx[1] of the bank hold the voxel-ordered scan afterwards (key_mode 2: see VoxelPlan)
int enqueue_voxel_sort(fdm_engine* e, const RayLane& lane, const VoxelPlan& plan, unsigned n, float voxel_size,
                       int flag_slot, const float* dx, const float* dy, const float* dz) {
  RayBank& b = lane.b;
  const float inv = 1.0f / voxel_size;  // voxel_grid_impl.hpp:46
  const VoxelCompact& C = plan.C;
  const bool compact = plan.key_mode != 0;  // true: uint32 keys
  if (e->opt.voxel_any_order) {  // the order std::sort leaves (fdm_introsort.hpp)
    if (compact) {
      launch_voxel_keys<uint32_t>(e, lane, n, inv, flag_slot, C, dx, dy, dz, 0);
      return enqueue_introsort<uint32_t>(lane, n);
    }
    launch_voxel_keys<unsigned long long>(e, lane, n, inv, flag_slot, C, dx, dy, dz, 0);
    return enqueue_introsort<unsigned long long>(lane, n);
  }
  if (plan.key_mode == 2) {
    // small scans: no sort at all (k_vs_*: fdm_raycast.hpp).  vkeys[0] = keys by point | places by point, vs_rec =
    // {key, point, bucket start, bucket size} by position; k_vs_mark runs from enqueue_ray_walk
    VoxelSmall& V = e->vs;
    // fine buckets = one (z, y) row of voxels when that fits 2^18 counters, else the key's top 18 bits
    V.shift = unsigned(std::max(C.bits, plan.key_bits - int(kVsFineBits)));
    V.fine = e->vs_cnt;
    V.coarse = e->vs_cnt + (size_t(1) << kVsFineBits);
    V.total = V.coarse + kVsCoarse;
    uint32_t* k0 = reinterpret_cast<uint32_t*>(b.vkeys[0]);
    V.place = k0 + b.vcap;                                   // (vkeys[0] holds 2 x vcap uint32)
    V.rec = e->vs_rec;
    V.cap = unsigned(e->vs_rec_cap);
    V.ibits = 1u;
    V.dbg = (e->opt.dbg_ray >> 8) & 3;
    while ((1u << V.ibits) < n) ++V.ibits;
    const unsigned blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_vs_count, dim3(blocks), dim3(256), 0, lane.s, n, inv, flag_slot, C, V, e->d_state, dx, dy,
                       dz, k0, b.vsel);
    hipLaunchKernelGGL(k_vs_scatter, dim3(blocks), dim3(256), 0, lane.s, n, V, k0);
    HIPCK(hipGetLastError());
    return FDM_OK;
  }
  // compact keys: bits 3*bits .. 31 are zero in every valid key and one in the invalid key (all ones): sorting
  // one bit past the fields is enough to keep the dropped points behind every voxel
  const unsigned sort_bits = C.bits > 0 ? unsigned(plan.key_bits + 1) : 64u;
  const int src = voxel_sort_source(sort_bits);
  if (compact) {
    launch_voxel_keys<uint32_t>(e, lane, n, inv, flag_slot, C, dx, dy, dz, src);
    HIPCK(hipGetLastError());
    return enqueue_radix_sort<uint32_t>(lane, n, sort_bits);
  }
  launch_voxel_keys<unsigned long long>(e, lane, n, inv, flag_slot, C, dx, dy, dz, src);
  HIPCK(hipGetLastError());
  return enqueue_radix_sort<unsigned long long>(lane, n, sort_bits);
}

fdm_raycast_config ray_config_of(const fdm_config& c) {
  fdm_raycast_config r;
  r.enabled = c.raycast_enabled;
  r.height_conflict_threshold = c.rc_height_conflict_threshold;
  r.log_odds_observed = c.rc_log_odds_observed;
  r.log_odds_ghost = c.rc_log_odds_ghost;
  r.log_odds_max = c.rc_log_odds_max;
  r.clear_threshold = c.rc_clear_threshold;
  return r;
}

RayParams make_ray_params(fdm_engine* e, const fdm_raycast_config& c, const float* origin, unsigned n,
                          int slot, int flag_slot) {
  RayParams Q{};
  Q.ox = origin[0]; Q.oy = origin[1]; Q.oz = origin[2];
  Q.l_obs = c.log_odds_observed;
  Q.l_ghost = c.log_odds_ghost;
  Q.l_max = c.log_odds_max;
  Q.clear_thr = c.clear_threshold;
  Q.conflict_thr = c.height_conflict_threshold;
  Q.resolution = static_cast<float>(e->G.res);
  Q.inv_voxel = 1.0f / Q.resolution;
  Q.n = n;
  Q.slot = slot;
  Q.flag_slot = flag_slot;
  Q.vis_stamp = 3u * unsigned(e->scan_no) + (flag_slot >= 0 ? 3u : 1u);
  Q.dbg = e->opt.dbg_ray;
  Q.by_sector = 0;
  Q.ctx = 0;
  Q.pre_slot = -1;
  Q.pre_do_move = Q.pre_gate = 0;
  return Q;
}

// ---- the stage: processScan (mark, ray queue, walk), then resolveGhostCells ----
// Everything of a stage up to the walk, in the lane's bank on the lane's stream (the bank: ensure_ray_cells and
// ensure_voxel_buffers(Q.n) — vidx[0] doubles as the ray queue).  voxel: the points are the bank's vkeys[1] / vidx[1]
// runs, as enqueue_voxel_sort left them (key_mode).
int enqueue_ray_walk(fdm_engine* e, const RayLane& lane, const RayParams& Q_in, bool voxel, const float* dx,
                     const float* dy, const float* dz, int key_mode) {
  if (!find_layer(e, "elevation")) return FDM_OK;  // raycasting.cpp:213-216
  RayBank& b = lane.b;
  int rc;
  RayParams Q = Q_in;
  const unsigned blocks = (Q.n + 255u) / 256u;
  uint32_t* ray_list = b.vidx[0];
  if (voxel && key_mode == 2) {
    hipLaunchKernelGGL(k_vs_mark, dim3(blocks), dim3(256), 0, lane.s, e->vs, b.vsel);
  } else if (voxel) {
    if (key_mode == 1)
      hipLaunchKernelGGL(k_voxel_mark<uint32_t>, dim3(blocks), dim3(256), 0, lane.s, Q.n,
                         reinterpret_cast<const uint32_t*>(b.vkeys[1]), b.vidx[1], b.vsel);
    else
      hipLaunchKernelGGL(k_voxel_mark<unsigned long long>, dim3(blocks), dim3(256), 0, lane.s, Q.n,
                         b.vkeys[1], b.vidx[1], b.vsel);
  }
  // large scans: queue bucketed by (wedge, length class) before the walk (see k_ray_compact)
  const bool large = Q.n >= unsigned(e->opt.ray_large_min);  // one lane per ray, queue bucketed by (wedge, length)
  const bool sort_queue = large && !(e->opt.dbg_ray & 2048);
  // large scans walk with an angular sector's minimum-height image in LDS (fdm_raywedge.hpp): the queue is ordered
  // (sector, length class) for it
  const bool wedge = sort_queue && e->opt.ray_wedge != 0;
  if (wedge) Q.by_sector = 1;
  uint32_t* ray_key = sort_queue ? reinterpret_cast<uint32_t*>(b.vkeys[0]) : nullptr;       // vkeys hold 2 x vcap uint32
  uint32_t* ray_rank = sort_queue ? reinterpret_cast<uint32_t*>(b.vkeys[0]) + b.vcap : nullptr;
  uint32_t* bin_cnt = sort_queue ? b.ray_bins : nullptr;
  if (sort_queue) {
    // points per thread of the queue builder: 8 on multi-million-point scans (the queue tail is one same-address
    // returning atomic per block), 2 below (a 272 K-point scan is 133 blocks of 2 048 points: half the chip)
    unsigned queue_blocks = 0u, queue_block_points = 0u;  // the queue builder's grid: the scatter walks the same block regions
    auto compact = [&](auto PTS) {
      constexpr unsigned kPts = decltype(PTS)::value;
      const unsigned cblocks = (Q.n + 256u * kPts - 1u) / (256u * kPts);
      if (voxel)
        hipLaunchKernelGGL((k_ray_compact<true, int(kPts)>), dim3(cblocks), dim3(256), 0, lane.s, Q, e->G, e->d_state,
                           dx, dy, dz, b.vsel, b.rc_cnt, ray_list, ray_key, ray_rank, bin_cnt, b.ray_blk);
      else
        hipLaunchKernelGGL((k_ray_compact<false, int(kPts)>), dim3(cblocks), dim3(256), 0, lane.s, Q, e->G, e->d_state,
                           dx, dy, dz, static_cast<const uint32_t*>(nullptr), b.rc_cnt, ray_list, ray_key, ray_rank,
                           bin_cnt, b.ray_blk);
      queue_blocks = cblocks;
      queue_block_points = 256u * kPts;
    };
    if (Q.n <= kRsSmallMax) compact(std::integral_constant<unsigned, 2>{});
    else compact(std::integral_constant<unsigned, 8>{});
    uint32_t* bin_start = b.ray_bins + kRayBins;
    uint32_t* bin_part = b.ray_bins + 2u * kRayBins;
    static_assert(kRaySectors * kRaySectorClasses == kRayScan1Threads * kRayScan1Per,
                  "k_ray_bin_scan1 scans every (sector, length class) bucket");
    if (wedge) {
      hipLaunchKernelGGL(k_ray_bin_scan1, dim3(1), dim3(kRayScan1Threads), 0, lane.s, Q, e->G, e->d_state, bin_cnt,
                         bin_start);
    } else {
      hipLaunchKernelGGL(k_ray_bin_sum, dim3(kRayBins / kRayBinBlock), dim3(256), 0, lane.s, Q, e->G, e->d_state,
                         bin_cnt, bin_part);
      hipLaunchKernelGGL(k_ray_bin_scan, dim3(kRayBins / kRayBinBlock), dim3(256), 0, lane.s, Q, e->G, e->d_state,
                         bin_cnt, bin_part, bin_start);
    }
    hipLaunchKernelGGL(k_ray_scatter, dim3(queue_blocks), dim3(256), 0, lane.s, Q, e->G, e->d_state, ray_list, ray_key,
                       ray_rank, bin_start, b.ray_blk, queue_block_points, b.vidx[1]);
    ray_list = b.vidx[1];
  } else if (voxel) {
    hipLaunchKernelGGL((k_ray_compact<true, 1>), dim3(blocks), dim3(256), 0, lane.s, Q, e->G, e->d_state, dx,
                       dy, dz, b.vsel, b.rc_cnt, ray_list, ray_key, ray_rank, bin_cnt, static_cast<uint32_t*>(nullptr));
  } else {
    hipLaunchKernelGGL((k_ray_compact<false, 1>), dim3(blocks), dim3(256), 0, lane.s, Q, e->G, e->d_state, dx,
                       dy, dz, static_cast<const uint32_t*>(nullptr), b.rc_cnt, ray_list, ray_key, ray_rank, bin_cnt,
                       static_cast<uint32_t*>(nullptr));
  }
  HIPCK(hipGetLastError());
  const bool tiled = e->G.o_rows != e->G.rows || e->G.o_cols != e->G.cols || e->G.s_rows != e->G.rows ||
                     e->G.s_cols != e->G.cols;
  auto launch_ray = [&](auto kern, unsigned seg) {
    // upper bound of the queue: every point a ray, padded to whole wavefronts per segment
    const unsigned threads = ((Q.n + 63u) & ~63u) * seg;
    hipLaunchKernelGGL(kern, dim3((threads + 255u) / 256u), dim3(256), 0, lane.s, Q, e->G, e->d_state, dx, dy,
                       dz, ray_list, b.rc_min);
  };
  // small scans are a few hundred wavefronts of dependent round trips: 16 / 8 lanes share a ray
  // (C2: k_ray 60 -> 25 (8) -> 16 us (16)); the point count bounds the ray count from above
  if (wedge) {
    const unsigned H = std::min(unsigned(std::max(e->G.rows, e->G.cols)) + 2u, kRwRowsMax);
    const unsigned lds = H * kRwCols * unsigned(sizeof(uint32_t));
    // one workgroup per sector; a sector of a very dense scan is shared by several (each flushes its own window)
    const unsigned sectors = kRaySectors;
    // (a camera's 60-degree field of view puts its rays into 43 of the 256 sectors; four workgroups per sector for
    // scans of that size measured 22 us against 18: every one initialises and flushes a window of its own)
    const unsigned parts = std::max(1u, std::min(8u, Q.n / (sectors * 8u * kRwThreads)));
    const uint32_t* bin_start = b.ray_bins + kRayBins;
    auto launch_wedge = [&](auto kern) -> int {
      if (int rc_lds = allow_lds(kern, lds)) return rc_lds;
      hipLaunchKernelGGL(kern, dim3(sectors * parts), dim3(kRwThreads), lds, lane.s, Q, e->G, e->d_state, dx, dy, dz,
                         ray_list, bin_start, b.rc_min, H, parts);
      return FDM_OK;
    };
    const bool fwin = !(e->opt.dbg_ray & (1 << 20));  // (dbg_ray 1048576, measurement only: the integer window of round 5)
    if (tiled) rc = fwin ? launch_wedge(k_ray_wedge<true, true>) : launch_wedge(k_ray_wedge<true, false>);
    else rc = fwin ? launch_wedge(k_ray_wedge<false, true>) : launch_wedge(k_ray_wedge<false, false>);
    if (rc) return rc;
  } else if (Q.n < (1u << 16) && !large) {
    tiled ? launch_ray(k_ray<true, 16>, 16u) : launch_ray(k_ray<false, 16>, 16u);
  } else if (!large) {
    tiled ? launch_ray(k_ray<true, 8>, 8u) : launch_ray(k_ray<false, 8>, 8u);
  } else {
    tiled ? launch_ray(k_ray<true, 1>, 1u) : launch_ray(k_ray<false, 1>, 1u);
  }
  HIPCK(hipGetLastError());
  return FDM_OK;
}

// resolveGhostCells on what a walk left in the lane's bank
RayLayers ray_layers_of(fdm_engine* e, const Layer& elev) {
  RayLayers L{};
  L.elevation = lptr(e, elev);
  L.elevation_stride = lstride(e, elev);
  L.logodds = find_layer(e, "_visibility_logodds")->d;
  L.ray_min = find_layer(e, "raycasting")->d;
  L.ghost = find_layer(e, "ghost_removal")->d;
  L.rec = e->d_rec;
  L.rec_floats = e->rec_floats;
  return L;
}
int enqueue_ray_resolve(fdm_engine* e, const RayLane& lane, const RayParams& Q) {
  const Layer* elev = find_layer(e, "elevation");
  if (!elev) return FDM_OK;
  const RayLayers L = ray_layers_of(e, *elev);
  hipLaunchKernelGGL(k_ray_resolve, dim3(unsigned((e->ncell + 255) / 256)), dim3(256), 0, lane.s, Q, e->G, e->d_state, L,
                     e->d_layer_ptrs, e->n_layer_ptrs, lane.b.rc_cnt, lane.b.rc_min, unsigned(e->ncell));
  HIPCK(hipGetLastError());
  return FDM_OK;
}

// The raycasting stage of a scan of integrate(), on the map its update — launched just before — leaves: voxel filter
// of the scan's preprocessed cloud, processScan, resolveGhostCells.  Everything it needs was fixed when the scan was
// enqueued (PendingUpdate::RQ, the cloud of the scan's parity): it may run after the NEXT scan's bin half.
// Option "ray_overlap": the part of a large scan's stage that needs the scan and the map GEOMETRY only — voxel filter,
// ray queue, walk — is launched when the scan's bin half has been, in the bank of the scan's parity on that bank's stream,
// with the geometry derived as the update will commit it (RayParams::pre_slot).  Stages of consecutive scans then run beside
// each other (and beside the fused launches of the main stream); k_ray_resolve stays where it was: behind the scan's
// update, ahead of the next one, on the main stream, which waits for the early part there.
int ensure_ray_streams(fdm_engine* e) {
  if (e->ray_bank[0].stream) return FDM_OK;
  for (RayBank& b : e->ray_bank) {
    HIPCK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
    HIPCK(hipEventCreateWithFlags(&b.ev_pre, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&b.ev_res, hipEventDisableTiming));
  }
  HIPCK(hipEventCreateWithFlags(&e->ev_ray_bin, hipEventDisableTiming));
  return FDM_OK;
}
int start_ray_stage_early(fdm_engine* e, fdm_engine::PendingUpdate& u, const ScanParams& P) {
  u.ray_pre = 0;
  const bool want = e->opt.ray_overlap > 0 || (e->opt.ray_overlap < 0 && (e->sync_call || u.RQ.n >= 1000000u));
  if (!want || !u.ray || u.RQ.n < unsigned(e->opt.ray_large_min) || e->profile || !e->opt.ray_wedge) return FDM_OK;
  if (e->opt.voxel_small && !e->opt.voxel_any_order && u.RQ.n <= unsigned(e->opt.voxel_small_max))
    return FDM_OK;  // (the sort-free filter keeps state of its own, on the engine: main stream only)
  if (!find_layer(e, "elevation")) return FDM_OK;
  int rc;
  if ((rc = ensure_ray_streams(e))) return rc;
  const int ctx = int(P.scan_no & 1u);
  RayBank& b = e->ray_bank[ctx];
  const float voxel_size = static_cast<float>(e->G.res);
  const VoxelPlan plan = plan_voxel_sort(e, u.RQ.n, voxel_size, u.ray_box);
  // The bank first, on the main stream.  Growing it drains the streams and, with them, flushes this very scan: its
  // stage has then run whole, in bank 0 (run_held_ray_stage), and there is nothing left to start
  const bool fresh = !b.rc_cnt || u.RQ.n > b.vcap || (e->opt.voxel_any_order && u.RQ.n > b.is_cap);
  if ((rc = ensure_ray_cells(e, b)) || (rc = ensure_voxel_sort(e, b, u.RQ.n, plan))) return rc;
  if (!u.ray || !e->chain) return FDM_OK;
  const RayLane lane{b, b.stream};
  // the scan's bin half (and everything before it): marked right behind that launch (enqueue_scan) — a mark taken here
  // would also wait for the previous scan's stage, whose resolve has been put on the main stream since.  A fresh bank's
  // fills are on the main stream behind that mark: a new one
  if (fresh || !e->ray_bin_marked) HIPCK(hipEventRecord(e->ev_ray_bin, e->stream));
  HIPCK(hipStreamWaitEvent(lane.s, e->ev_ray_bin, 0));
  if (b.res_pending) HIPCK(hipStreamWaitEvent(lane.s, b.ev_res, 0));  // the bank's previous stage has been resolved
  RayParams Q = u.RQ;
  Q.ctx = ctx;
  Q.pre_slot = P.slot;
  Q.pre_do_move = P.do_move;
  Q.pre_gate = P.gate_on_filter;
  if ((rc = enqueue_voxel_sort(e, lane, plan, Q.n, voxel_size, Q.flag_slot, u.ray_x, u.ray_y, u.ray_z))) return rc;
  if ((rc = enqueue_ray_walk(e, lane, Q, true, u.ray_x, u.ray_y, u.ray_z, plan.key_mode))) return rc;
  HIPCK(hipEventRecord(b.ev_pre, lane.s));
  u.RQ = Q;
  u.ray_pre = 1 + ctx;
  return FDM_OK;
}

int run_held_ray_stage(fdm_engine* e, fdm_engine::PendingUpdate& u) {
  if (!u.ray) return FDM_OK;
  u.ray = false;
  int rc;
  if (u.ray_pre) {  // the first part is on its way (start_ray_stage_early): wait for it here, resolve
    RayBank& b = e->ray_bank[u.ray_pre - 1];
    u.ray_pre = 0;
    HIPCK(hipStreamWaitEvent(e->stream, b.ev_pre, 0));
    if ((rc = enqueue_ray_resolve(e, RayLane{b, e->stream}, u.RQ))) return rc;
    HIPCK(hipEventRecord(b.ev_res, e->stream));
    b.res_pending = true;
    e->ray_timed = false;
    return FDM_OK;
  }
  // the normal path: the whole stage in bank 0 on the main stream
  const RayLane lane{e->ray_bank[0], e->stream};
  const float voxel_size = static_cast<float>(e->G.res);
  const VoxelPlan plan = plan_voxel_sort(e, u.RQ.n, voxel_size, u.ray_box);
  if ((rc = ensure_ray_cells(e, lane.b)) || (rc = ensure_voxel_sort(e, lane.b, u.RQ.n, plan))) return rc;
  if (e->profile) HIPCK(hipEventRecord(e->ev_ray[0], e->stream));
  if ((rc = enqueue_voxel_sort(e, lane, plan, u.RQ.n, voxel_size, u.RQ.flag_slot, u.ray_x, u.ray_y, u.ray_z))) return rc;
  if ((rc = enqueue_ray_walk(e, lane, u.RQ, true, u.ray_x, u.ray_y, u.ray_z, plan.key_mode))) return rc;
  if ((rc = enqueue_ray_resolve(e, lane, u.RQ))) return rc;
  // (option "ray_overlap": the next early stage of bank 0 may already be waiting only for a bin half enqueued AHEAD of
  //  this stage (enqueue_scan's ev_ray_bin): it waits for this mark too)
  if (lane.b.stream) {
    HIPCK(hipEventRecord(lane.b.ev_res, e->stream));
    lane.b.res_pending = true;
  }
  if (e->profile) {
    HIPCK(hipEventRecord(e->ev_ray[1], e->stream));
    e->ray_timed = true;
  }
  return FDM_OK;
}

}  // namespace fdmh

extern "C" {

// ---- raycasting entry points ----
int fdm_engine_apply_raycasting_device(fdm_engine* e, uint64_t n, const float* dx, const float* dy,
                                       const float* dz, const float origin[3],
                                       const fdm_raycast_config* rcfg) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !origin) return fail(FDM_ERR_INVALID, "null argument");
  const fdm_raycast_config c = rcfg ? *rcfg : ray_config_of(e->cfg);
  if (!c.enabled || n == 0) return FDM_OK;  // raycasting.cpp:207-209
  if (!dx || !dy || !dz) return fail(FDM_ERR_INVALID, "null xyz");
  if (n >= 0xFFFFFFFEull) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-2");
  HIPCK(hipSetDevice(e->device));
  int rc;
  if (!find_layer(e, "elevation")) return FDM_OK;
  if ((rc = ensure_ray_layers(e))) return rc;
  if ((rc = refresh_layer_ptrs(e))) return rc;
  const RayParams Q = make_ray_params(e, c, origin, unsigned(n), int(e->scan_no & 3), -1);
  const RayLane lane{e->ray_bank[0], e->stream};
  if ((rc = ensure_ray_cells(e, lane.b)) || (rc = ensure_voxel_buffers(e, lane.b, Q.n))) return rc;
  if ((rc = enqueue_ray_walk(e, lane, Q, false, dx, dy, dz, 0))) return rc;
  return enqueue_ray_resolve(e, lane, Q);
}

int fdm_engine_apply_raycasting(fdm_engine* e, uint64_t n, const float* x, const float* y,
                                const float* z, const float origin[3], const fdm_raycast_config* rcfg) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !origin) return fail(FDM_ERR_INVALID, "null argument");
  if (!(rcfg ? rcfg->enabled : e->cfg.raycast_enabled) || n == 0) return FDM_OK;
  if (!x || !y || !z) return fail(FDM_ERR_INVALID, "null xyz");
  HIPCK(hipSetDevice(e->device));
  ScanInputs dev;
  int rc = stage_inputs(e, n, {x, y, z}, &dev);
  if (rc) return rc;
  if ((rc = fdm_engine_apply_raycasting_device(e, n, dev.x, dev.y, dev.z, origin, rcfg))) return rc;
  if (int rc_sync = sync_all(e)) return rc_sync;
  return FDM_OK;
}

int fdm_engine_voxel_any(fdm_engine* e, uint64_t n, const float* x, const float* y, const float* z,
                         float voxel_size, uint32_t* out_idx, uint64_t* n_out) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !n_out) return fail(FDM_ERR_INVALID, "null argument");
  *n_out = 0;
  if (!voxel_size_ok(voxel_size)) return fail(FDM_ERR_INVALID, "voxel_size must be in [0.001, 100]");
  if (n == 0) return FDM_OK;
  if (!x || !y || !z || !out_idx) return fail(FDM_ERR_INVALID, "null argument");
  if (n >= 0xFFFFFFFEull) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-2");
  HIPCK(hipSetDevice(e->device));
  ScanInputs dev;
  int rc = stage_inputs(e, n, {x, y, z}, &dev);
  if (rc) return rc;
  const RayLane lane{e->ray_bank[0], e->stream};
  const VoxelPlan plan = plan_voxel_sort(e, unsigned(n), voxel_size, nullptr);  // no box: full 63-bit keys
  if ((rc = ensure_voxel_sort(e, lane.b, unsigned(n), plan))) return rc;
  if ((rc = enqueue_voxel_sort(e, lane, plan, unsigned(n), voxel_size, -1, dev.x, dev.y, dev.z))) return rc;
  hipLaunchKernelGGL(k_voxel_select, dim3(unsigned((n + 255) / 256)), dim3(256), 0, e->stream, unsigned(n),
                     lane.b.vkeys[1], lane.b.vidx[1], lane.b.vsel);
  HIPCK(hipGetLastError());
  std::vector<uint32_t> h(n);
  HIPCK(hipMemcpyAsync(h.data(), lane.b.vsel, n * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  if (int rc_sync = sync_all(e)) return rc_sync;
  uint64_t w = 0;
  for (uint64_t i = 0; i < n; ++i)  // order-preserving compaction = marshalling
    if (h[i] != kNoIdx) out_idx[w++] = h[i];
  *n_out = w;
  return FDM_OK;
}

int fdm_engine_last_ray_ms(fdm_engine* e, float* ms) {
  if (int rc = join_streams(e)) return rc;
  if (!e || !ms) return fail(FDM_ERR_INVALID, "null argument");
  if (!e->profile) return fail(FDM_ERR_INVALID, "profiling is off");
  *ms = 0.f;
  if (!e->ray_timed) return FDM_OK;
  if (int rc_sync = sync_all(e)) return rc_sync;
  HIPCK(hipEventElapsedTime(ms, e->ev_ray[0], e->ev_ray[1]));
  return FDM_OK;
}


}  // extern "C"
