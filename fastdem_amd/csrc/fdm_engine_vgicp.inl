// fdm_engine_vgicp.inl — host side of voxelized GICP (kernels: fdm_vgicp.hpp): the voxel distribution map as a handle that
// outlives a call — fdm_voxel_map_create, _destroy, _get_info, _records (struct fdm_voxel_map itself is stated in
// fdm_engine_register.inl, which reads it) — and the two entries that register against it, fdm_cloud_register_vgicp and
// fdm_cloud_register_vgicp_linearize: they pack a RegProblem whose target is the map and call the one registration path
// of fdm_engine_register.inl (reg_align, reg_linearize), as the cloud entries do.  Part of fdm_engine_post.hip, behind
// fdm_engine_register.inl and fdm_engine_segment.inl (SortBufs64).  Engine-free like the other cloud calls: a call picks
// the device, works on the null stream and is synchronous; the build's scratch is freed when create returns, the map
// keeps its records and its table.

namespace {
void vg_free(fdm_voxel_map* m) {
  if (!m) return;
  if (m->rec_mem || m->table_mem) {
    const ScopedDevice restore;
    if (hipSetDevice(m->info.device) == hipSuccess) {
      if (m->rec_mem) (void)hipFree(m->rec_mem);
      if (m->table_mem) (void)hipFree(m->table_mem);
    }
  }
  delete m;
}
struct VgOwner {  // a map under construction: destroyed unless released
  fdm_voxel_map* m = nullptr;
  ~VgOwner() { vg_free(m); }
  fdm_voxel_map* release() {
    fdm_voxel_map* const r = m;
    m = nullptr;
    return r;
  }
};
size_t vg_round(size_t bytes) { return (bytes + 255u) & ~size_t(255); }

// `device` is current; n > 0
int vg_build(fdm_voxel_map* m, uint64_t n, const float* x, const float* y, const float* z, bool on_device) {
  hipStream_t s = nullptr;
  const unsigned np = unsigned(n);
  const unsigned blocks = (np + 255u) / 256u;
  const bool clock = cloud_profile_on();
  Events E;
  if (clock)
    if (int rc = E.init(4)) return rc;
  auto mark = [&](int k) { return clock ? hipEventRecord(E.ev[k], s) : hipSuccess; };

  CloudBlock b_in, b_stage;
  const float* in[3] = {};
  const void* const h_in[3] = {x, y, z};
  if (int rc = stage_cloud(s, n, 3, h_in, on_device, b_in, in)) return rc;
  SortBufs64 S;
  if (int rc = S.alloc(np)) return rc;
  DevBuf b_pos, b_counts, b_long, b_stat;
  if (int rc = b_stage.alloc(np, 3)) return rc;
  if (int rc = b_pos.alloc((size_t(np) + 1) * sizeof(uint32_t))) return rc;
  if (int rc = b_counts.alloc((size_t(blocks) + 1) * sizeof(uint32_t))) return rc;
  if (int rc = b_long.alloc((size_t(np / kVxLong) + 1) * sizeof(uint32_t))) return rc;
  if (int rc = b_stat.alloc(sizeof(VgStat))) return rc;
  VgStat* const d_stat = b_stat.as<VgStat>();
  HIPCK(hipMemsetAsync(d_stat, 0, sizeof(VgStat), s));

  // keys and the stable sort.  k_voxel_keys leaves the first pass's histogram, and clears a flag per point that only the
  // raycasting stage reads: the index side the first pass does not read takes those words
  HIPCK(mark(0));
  {
    const unsigned tile = rs_tile(np), tiles = (np + tile - 1u) / tile;
    const VoxelCompact none{0, 0, 0, 0, 0};  // the full 63-bit key
    if (tile == kRsTileSmall)
      hipLaunchKernelGGL((k_voxel_keys<unsigned long long, kRsTileSmall, false>), dim3(tiles), dim3(256), 0, s, np,
                         m->info.inv_resolution, -1, none, static_cast<DevState*>(nullptr), in[0], in[1], in[2],
                         S.pairs.keys[0], S.pairs.idx[0], tiles, S.pairs.hist);
    else
      hipLaunchKernelGGL((k_voxel_keys<unsigned long long, kRsTile, false>), dim3(tiles), dim3(256), 0, s, np,
                         m->info.inv_resolution, -1, none, static_cast<DevState*>(nullptr), in[0], in[1], in[2],
                         S.pairs.keys[0], S.pairs.idx[0], tiles, S.pairs.hist);
    HIPCK(hipGetLastError());
  }
  const int side = rs_enqueue(s, S.pairs, np, 64u, 0, kRsHistGiven);
  HIPCK(hipGetLastError());
  HIPCK(mark(1));

  // run heads -> voxels, and x, y, z in sorted order
  const unsigned long long* const keys = S.pairs.keys[side];
  const uint32_t* const idx = S.pairs.idx[side];
  uint32_t* const counts = b_counts.as<uint32_t>();
  uint32_t* const pos = b_pos.as<uint32_t>();
  const VxCloud C{in[0], in[1], in[2], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const VxStage G{b_stage.ch(0), b_stage.ch(1), b_stage.ch(2), nullptr, nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(k_vx_count, dim3(blocks), dim3(256), 0, s, np, keys, counts);
  hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, s, counts, blocks);
  hipLaunchKernelGGL(k_vx_heads, dim3(blocks), dim3(256), 0, s, np, keys, idx, counts, C, G, pos);
  HIPCK(hipGetLastError());
  uint32_t total = 0;
  HIPCK(hipMemcpyAsync(&total, counts + blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (total > np) return fail(FDM_ERR_HIP, "the run count overran the cloud");
  if (total == 0) {  // no finite point
    m->info.n_skipped = n;
    return FDM_OK;
  }
  uint32_t n_valid = 0;
  HIPCK(hipMemcpyAsync(&n_valid, pos + total, sizeof(uint32_t), hipMemcpyDeviceToHost, s));

  // the records
  const size_t nv = total;
  const size_t o_key = 0, o_creg = o_key + vg_round(nv * sizeof(unsigned long long));
  const size_t o_count = o_creg + vg_round(nv * 6 * sizeof(double)), o_mean = o_count + vg_round(nv * sizeof(uint32_t));
  const size_t o_cov = o_mean + vg_round(nv * 3 * sizeof(float)), bytes = o_cov + vg_round(nv * 9 * sizeof(float));
  HIPCK(hipMalloc(&m->rec_mem, bytes));
  char* const base = static_cast<char*>(m->rec_mem);
  m->R.key = reinterpret_cast<unsigned long long*>(base + o_key);
  m->R.creg6 = reinterpret_cast<double*>(base + o_creg);
  m->R.count = reinterpret_cast<uint32_t*>(base + o_count);
  m->R.mean3 = reinterpret_cast<float*>(base + o_mean);
  m->R.cov9 = reinterpret_cast<float*>(base + o_cov);
  const double eps = m->info.covariance_epsilon;
  hipLaunchKernelGGL(k_vg_reduce, dim3((total + 255u) / 256u), dim3(256), 0, s, total, pos, keys, G.x, G.y, G.z, eps, m->R,
                     d_stat, b_long.as<uint32_t>());
  if (np > kVxLong)  // (at most np / kVxLong long runs)
    hipLaunchKernelGGL(k_vg_reduce_long, dim3(std::min(np / kVxLong, 2048u)), dim3(64), 0, s, b_long.as<uint32_t>(), pos,
                       keys, G.x, G.y, G.z, eps, m->R, d_stat);
  HIPCK(hipGetLastError());
  HIPCK(mark(2));

  // the table: a power of two of at least 2 * num_voxels slots
  unsigned long long slots = 2;
  while (slots < 2ull * nv) slots <<= 1;
  HIPCK(hipMalloc(&m->table_mem, size_t(slots) * (sizeof(unsigned long long) + sizeof(uint32_t))));
  unsigned long long* const slot_key = static_cast<unsigned long long*>(m->table_mem);
  uint32_t* const slot_rank = reinterpret_cast<uint32_t*>(slot_key + slots);
  HIPCK(hipMemsetAsync(slot_key, 0xFF, size_t(slots) * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_vg_insert, dim3((total + 255u) / 256u), dim3(256), 0, s, total, m->R.key, slot_key, slot_rank,
                     slots - 1ull, d_stat);
  HIPCK(hipGetLastError());
  HIPCK(mark(3));
  VgStat hs{};
  HIPCK(hipMemcpyAsync(&hs, d_stat, sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (hs.max_probe == 0u || hs.max_probe > total) return fail(FDM_ERR_HIP, "the voxel table's probe length is out of range");

  m->info.n_skipped = n - n_valid;
  m->info.num_voxels = nv;
  m->info.n_sparse = hs.n_sparse;
  m->info.max_count = hs.max_count;
  m->info.max_probe = hs.max_probe;
  m->info.table_slots = slots;
  if (clock)
    for (int q = 0; q < 3; ++q) m->info.ms[q] = E.ms(q, q + 1);
  m->T = VgTable{slot_key, slot_rank, slots - 1ull, hs.max_probe, m->info.inv_resolution, m->R.mean3, m->R.creg6};
  return FDM_OK;
}

// a registration against `map`, on its device
RegProblem vg_problem(const fdm_voxel_map* map, uint64_t n, const float* sx, const float* sy, const float* sz,
                      const float* s_cov9, int on_device) {
  RegProblem P;
  P.method = kRegVGICP;
  P.voxels = true;
  P.map = map;
  P.device = map ? map->info.device : 0;
  P.n = n;
  P.x = sx; P.y = sy; P.z = sz;
  P.cov9 = s_cov9;
  P.on_device = on_device != 0;
  return P;
}
}  // namespace

extern "C" {

int fdm_voxel_map_create(uint64_t n, const float* x, const float* y, const float* z, int on_device, float resolution,
                         double covariance_epsilon, int device, fdm_voxel_map** out) {
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  *out = nullptr;
  const float inv = 1.0f / resolution;  // voxel_distribution_map.hpp:76
  if (!(resolution > 0.0f) || !std::isfinite(resolution) || !(inv > 0.0f) || !std::isfinite(inv))
    return fail(FDM_ERR_INVALID, "resolution and 1 / resolution must be positive and finite");
  if (!(covariance_epsilon >= 0.0)) return fail(FDM_ERR_INVALID, "covariance_epsilon must not be negative or NaN");
  // (the sorts count their tiles of up to 4 096 pairs, and every kernel here its blocks, in 32 bits: n + 4 096 must fit)
  if (n > 0xFFFFFFFFull - kRsTile) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-4097");
  if (n && (!x || !y || !z)) return fail(FDM_ERR_INVALID, "null coordinate array");
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  VgOwner own;
  own.m = new fdm_voxel_map;
  own.m->info.resolution = resolution;
  own.m->info.inv_resolution = inv;
  own.m->info.covariance_epsilon = covariance_epsilon;
  own.m->info.device = device;
  own.m->info.n_points = n;
  if (n)
    if (int rc = vg_build(own.m, n, x, y, z, on_device != 0)) return rc;
  *out = own.release();
  return FDM_OK;
}

void fdm_voxel_map_destroy(fdm_voxel_map* map) { vg_free(map); }

int fdm_voxel_map_get_info(const fdm_voxel_map* map, fdm_voxel_map_info* out) {
  if (!map || !out) return fail(FDM_ERR_INVALID, "null argument");
  *out = map->info;
  return FDM_OK;
}

int fdm_voxel_map_records(const fdm_voxel_map* map, int on_device, uint64_t* keys, float* mean3, float* cov9,
                          double* creg6, uint32_t* count) {
  if (!map) return fail(FDM_ERR_INVALID, "null argument");
  const size_t nv = size_t(map->info.num_voxels);
  if (nv == 0) return FDM_OK;
  const ScopedDevice restore;
  if (int rc = pick_device(map->info.device)) return rc;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (keys) HIPCK(hipMemcpy(keys, map->R.key, nv * sizeof(uint64_t), kind));
  if (mean3) HIPCK(hipMemcpy(mean3, map->R.mean3, nv * 3 * sizeof(float), kind));
  if (cov9) HIPCK(hipMemcpy(cov9, map->R.cov9, nv * 9 * sizeof(float), kind));
  if (creg6) HIPCK(hipMemcpy(creg6, map->R.creg6, nv * 6 * sizeof(double), kind));
  if (count) HIPCK(hipMemcpy(count, map->R.count, nv * sizeof(uint32_t), kind));
  if (on_device) HIPCK(hipDeviceSynchronize());
  return FDM_OK;
}

int fdm_cloud_register_vgicp(const fdm_voxel_map* map, uint64_t n_source, const float* sx, const float* sy,
                             const float* sz, const float* s_cov9, int on_device, const double* initial_guess,
                             const fdm_align_settings* settings, fdm_registration_result* out) {
  return reg_align(vg_problem(map, n_source, sx, sy, sz, s_cov9, on_device), initial_guess, settings, out);
}

int fdm_cloud_register_vgicp_linearize(const fdm_voxel_map* map, uint64_t n_source, const float* sx, const float* sy,
                                       const float* sz, const float* s_cov9, int on_device, const double* transform,
                                       const fdm_align_settings* settings, double H[21], double b[6], double* error,
                                       uint64_t* num_inliers, int32_t* corr) {
  return reg_linearize(vg_problem(map, n_source, sx, sy, sz, s_cov9, on_device), transform, settings, H, b, error,
                       num_inliers, corr);
}

}  // extern "C"
