// fdm_engine_voxel.inl — host side of the cloud downsampling filters (kernels: fdm_voxel.hpp): entry points
// fdm_cloud_voxel_grid, fdm_cloud_grid_max_z (and fdm_cloud_debug_profile / _last_ms, fdm_engine_debug.h).  Part of fdm_engine_ray.hip, behind
// fdm_engine_ray.inl, whose key launch, sort drivers and bank allocation it shares: the sort kernels are instantiated in
// this unit.  A cloud has no map and no engine: the call picks its device, works on the null stream in a RayBank and a
// scratch block of its own, and frees both on return.  Synchronous.

namespace {
struct ScopedBank {  // the sorts' buffers for one call
  RayBank b;
  ~ScopedBank() { b.release(); }
};
struct ScopedDev {
  void* p = nullptr;
  ~ScopedDev() { if (p) (void)hipFree(p); }
};
// fdm_cloud_debug_profile: the calling thread's calls are timed with four device events (none are created otherwise)
struct StageClock {
  hipEvent_t ev[4] = {};
  bool on = false;
  ~StageClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  int init(bool want) {
    on = want;
    if (on) for (hipEvent_t& e : ev) HIPCK(hipEventCreate(&e));
    return FDM_OK;
  }
  int mark(int k, hipStream_t s) {
    if (on) HIPCK(hipEventRecord(ev[k], s));
    return FDM_OK;
  }
};
thread_local bool g_downsample_profile = false;
thread_local float g_downsample_ms[3] = {0.f, 0.f, 0.f};

// arrays carved out of one block, each 256-byte aligned: a first walk with base 0 counts, the second hands out
struct Carver {
  uintptr_t base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* const p = reinterpret_cast<T*>(base + off);
    off += (count * sizeof(T) + 255u) & ~size_t(255);
    return p;
  }
};

// everything a call keeps on the device besides the bank: the staged input and the output of a host cloud, the sorted
// copies of the channels the mode walks, the run heads and the block counts
struct VxPlan {
  VxCloud in{};      // device input
  VxOut out{};       // device output
  VxStage stage{};
  uint32_t* pos = nullptr;
  uint32_t* counts = nullptr;
  uint32_t* long_count = nullptr;  // runs of more than kVxLong entries: how many, and their slots
  uint32_t* long_list = nullptr;
};
size_t vx_layout(uintptr_t base, size_t n, unsigned blocks, int mode, bool host, const fdm_cloud_view& V,
                 const fdm_cloud_out& O, VxPlan* P) {
  Carver c{base};
  const bool nrm = V.nx != nullptr;
  if (host) {
    P->in.x = c.take<float>(n); P->in.y = c.take<float>(n); P->in.z = c.take<float>(n);
    P->in.intensity = V.intensity ? c.take<float>(n) : nullptr;
    P->in.rgb = V.rgb ? c.take<uint32_t>(n) : nullptr;
    P->in.nx = nrm ? c.take<float>(n) : nullptr;
    P->in.ny = nrm ? c.take<float>(n) : nullptr;
    P->in.nz = nrm ? c.take<float>(n) : nullptr;
    P->in.cov9 = V.cov9 ? c.take<float>(9 * n) : nullptr;
    P->out.x = O.x ? c.take<float>(n) : nullptr;
    P->out.y = O.y ? c.take<float>(n) : nullptr;
    P->out.z = O.z ? c.take<float>(n) : nullptr;
    P->out.intensity = (O.intensity && V.intensity) ? c.take<float>(n) : nullptr;
    P->out.rgb = (O.rgb && V.rgb) ? c.take<uint32_t>(n) : nullptr;
    P->out.nx = (O.nx && nrm) ? c.take<float>(n) : nullptr;
    P->out.ny = (O.ny && nrm) ? c.take<float>(n) : nullptr;
    P->out.nz = (O.nz && nrm) ? c.take<float>(n) : nullptr;
    P->out.cov9 = (O.cov9 && V.cov9) ? c.take<float>(9 * n) : nullptr;
    P->out.idx = O.idx ? c.take<uint32_t>(n) : nullptr;
  } else {
    P->in = VxCloud{V.x, V.y, V.z, V.intensity, V.rgb, V.nx, V.ny, V.nz, V.cov9};
    P->out = VxOut{O.x, O.y, O.z, O.intensity, O.rgb, O.nx, O.ny, O.nz, O.cov9, O.idx};
  }
  const bool mean = mode == kVxCentroid || mode == kVxCenter;
  const bool xyz = mode == kVxCentroid || mode == kVxNearest;
  P->stage.x = xyz ? c.take<float>(n) : nullptr;
  P->stage.y = xyz ? c.take<float>(n) : nullptr;
  P->stage.z = (xyz || mode == kVxMaxZ) ? c.take<float>(n) : nullptr;
  P->stage.intensity = (mean && V.intensity) ? c.take<float>(n) : nullptr;
  P->stage.rgb = (mean && V.rgb) ? c.take<uint32_t>(n) : nullptr;
  P->stage.nx = (mean && nrm) ? c.take<float>(n) : nullptr;
  P->stage.ny = (mean && nrm) ? c.take<float>(n) : nullptr;
  P->stage.nz = (mean && nrm) ? c.take<float>(n) : nullptr;
  P->pos = c.take<uint32_t>(n + 1);
  P->counts = c.take<uint32_t>(size_t(blocks) + 1);
  P->long_count = c.take<uint32_t>(1);
  P->long_list = c.take<uint32_t>(n / kVxLong + 1);
  return c.off;
}

template <bool FLAT>
void launch_cloud_keys(const RayLane& lane, unsigned n, float inv, const float* dx, const float* dy, const float* dz,
                       int src) {
  const unsigned tile = rs_tile(n), tiles = (n + tile - 1u) / tile;
  const VoxelCompact none{0, 0, 0, 0, 0};  // the full 63-bit key
  if (tile == kRsTileSmall)
    hipLaunchKernelGGL((k_voxel_keys<unsigned long long, kRsTileSmall, FLAT>), dim3(tiles), dim3(256), 0, lane.s, n, inv,
                       -1, none, static_cast<DevState*>(nullptr), dx, dy, dz, lane.b.vkeys[src], lane.b.vsel, tiles,
                       lane.b.sort_tmp);
  else
    hipLaunchKernelGGL((k_voxel_keys<unsigned long long, kRsTile, FLAT>), dim3(tiles), dim3(256), 0, lane.s, n, inv, -1,
                       none, static_cast<DevState*>(nullptr), dx, dy, dz, lane.b.vkeys[src], lane.b.vsel, tiles,
                       lane.b.sort_tmp);
}

// the runs of up to kVxLong entries one lane each, the longer ones (at most n / kVxLong of them) one wavefront each
template <int MODE>
void launch_vx_reduce(hipStream_t s, unsigned n, unsigned n_out, const RayBank& b, const VxPlan& P, float size) {
  hipLaunchKernelGGL(k_vx_reduce<MODE>, dim3((n_out + 255u) / 256u), dim3(256), 0, s, n_out, P.pos, b.vkeys[1], b.vidx[1],
                     P.in, P.stage, size, P.out, P.long_count, P.long_list);
  if (MODE == kVxAny || n <= kVxLong) return;
  const unsigned waves = std::min(n / kVxLong, 2048u);
  hipLaunchKernelGGL(k_vx_reduce_long<MODE>, dim3(waves), dim3(64), 0, s, P.long_count, P.long_list, P.pos, b.vkeys[1],
                     b.vidx[1], P.in, P.stage, size, P.out);
}

// mode: VoxelMode, or kVxMaxZ
int cloud_downsample(uint64_t n, const fdm_cloud_view* in, int on_device, float size, int mode, int order, int device,
                     const fdm_cloud_out* out, uint64_t* n_out) {
  if (!n_out) return fail(FDM_ERR_INVALID, "null argument");
  *n_out = 0;
  g_downsample_ms[0] = g_downsample_ms[1] = g_downsample_ms[2] = 0.f;
  if (!voxel_size_ok(size))  // voxel_grid_impl.hpp:31-33, grid_max_z_impl.hpp:84-86 (a NaN passes neither comparison)
    return fail(FDM_ERR_INVALID, mode == kVxMaxZ ? "grid_size must be in [0.001, 100]" : "voxel_size must be in [0.001, 100]");
  if (order != 0 && order != 1) return fail(FDM_ERR_INVALID, "order must be 0 (stable) or 1 (std::sort)");
  // (the sorts count their tiles of up to 4 096 pairs, and every kernel here its blocks, in 32 bits: n + 4 096 must fit)
  if (n > 0xFFFFFFFFull - kRsTile) return fail(FDM_ERR_INVALID, "point count exceeds 2^32-4097");
  if (n == 0) return FDM_OK;
  if (!in || !in->x || !in->y || !in->z) return fail(FDM_ERR_INVALID, "null coordinate array");
  const int normals = int(in->nx != nullptr) + int(in->ny != nullptr) + int(in->nz != nullptr);
  if (normals != 0 && normals != 3) return fail(FDM_ERR_INVALID, "normals need all of nx, ny, nz");
  const fdm_cloud_view& V = *in;
  const fdm_cloud_out O = out ? *out : fdm_cloud_out{};
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  hipStream_t s = nullptr;
  const unsigned np = unsigned(n);
  const unsigned blocks = (np + 255u) / 256u;
  const bool host = on_device == 0;

  StageClock E;
  if (int rc = E.init(g_downsample_profile)) return rc;
  ScopedBank bank;
  ScopedDev mem;
  VxPlan P;
  int rc;
  if ((rc = alloc_voxel_buffers(bank.b, np))) return rc;
  if (order == 1 && (rc = alloc_introsort_buffers(bank.b, np))) return rc;
  HIPCK(hipMalloc(&mem.p, vx_layout(uintptr_t(0), np, blocks, mode, host, V, O, &P)));
  vx_layout(reinterpret_cast<uintptr_t>(mem.p), np, blocks, mode, host, V, O, &P);
  if (host) {
    auto up = [&](const void* dst, const void* src, size_t bytes) {
      return src ? hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    const size_t w = size_t(np) * sizeof(float);
    HIPCK(up(P.in.x, V.x, w)); HIPCK(up(P.in.y, V.y, w)); HIPCK(up(P.in.z, V.z, w));
    HIPCK(up(P.in.intensity, V.intensity, w)); HIPCK(up(P.in.rgb, V.rgb, w));
    HIPCK(up(P.in.nx, V.nx, w)); HIPCK(up(P.in.ny, V.ny, w)); HIPCK(up(P.in.nz, V.nz, w));
    HIPCK(up(P.in.cov9, V.cov9, 9 * w));
  }

  // keys and sort: vkeys[1] / vidx[1] hold the ordered pairs, the dropped points behind the valid ones
  const RayLane lane{bank.b, s};
  const float inv = 1.0f / size;  // voxel_grid_impl.hpp:46
  const bool flat = mode == kVxMaxZ;
  if ((rc = E.mark(0, s))) return rc;
  if (order == 1) {
    flat ? launch_cloud_keys<true>(lane, np, inv, P.in.x, P.in.y, P.in.z, 0)
         : launch_cloud_keys<false>(lane, np, inv, P.in.x, P.in.y, P.in.z, 0);
    HIPCK(hipGetLastError());
    if ((rc = enqueue_introsort<unsigned long long>(lane, np))) return rc;
  } else {
    // gridMaxZ: the z field of every valid key is that of index 0, 2^20 << 42 — bits 43 .. 63 are the same in all of them
    // and bit 42 is zero, while the invalid key has it set: the x and y fields and bit 42 order the pairs.  voxelGrid:
    // the whole key
    const unsigned bits = flat ? 43u : 64u;
    const int src = voxel_sort_source(bits);
    flat ? launch_cloud_keys<true>(lane, np, inv, P.in.x, P.in.y, P.in.z, src)
         : launch_cloud_keys<false>(lane, np, inv, P.in.x, P.in.y, P.in.z, src);
    HIPCK(hipGetLastError());
    if ((rc = enqueue_radix_sort<unsigned long long>(lane, np, bits))) return rc;
  }
  if ((rc = E.mark(1, s))) return rc;

  // run heads -> output slots, and the walked channels in sorted order
  const unsigned long long* keys = bank.b.vkeys[1];
  const uint32_t* idx = bank.b.vidx[1];
  hipLaunchKernelGGL(k_vx_count, dim3(blocks), dim3(256), 0, s, np, keys, P.counts);
  hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, s, P.counts, blocks);
  hipLaunchKernelGGL(k_vx_heads, dim3(blocks), dim3(256), 0, s, np, keys, idx, P.counts, P.in, P.stage, P.pos);
  HIPCK(hipGetLastError());
  if ((rc = E.mark(2, s))) return rc;
  uint32_t total = 0;
  HIPCK(hipMemcpyAsync(&total, P.counts + blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (total > np) return fail(FDM_ERR_HIP, "the run count overran the cloud");
  if (total) {
    HIPCK(hipMemsetAsync(P.long_count, 0, sizeof(uint32_t), s));
    switch (mode) {
      case kVxCentroid: launch_vx_reduce<kVxCentroid>(s, np, total, bank.b, P, size); break;
      case kVxNearest: launch_vx_reduce<kVxNearest>(s, np, total, bank.b, P, size); break;
      case kVxAny: launch_vx_reduce<kVxAny>(s, np, total, bank.b, P, size); break;
      case kVxCenter: launch_vx_reduce<kVxCenter>(s, np, total, bank.b, P, size); break;
      default: launch_vx_reduce<kVxMaxZ>(s, np, total, bank.b, P, size); break;
    }
    HIPCK(hipGetLastError());
  }
  if ((rc = E.mark(3, s))) return rc;
  if (host && total) {
    auto down = [&](void* dst, const void* src, size_t bytes) {
      return (dst && src) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    const size_t w = size_t(total) * sizeof(float);
    HIPCK(down(O.x, P.out.x, w)); HIPCK(down(O.y, P.out.y, w)); HIPCK(down(O.z, P.out.z, w));
    HIPCK(down(O.intensity, P.out.intensity, w)); HIPCK(down(O.rgb, P.out.rgb, w));
    HIPCK(down(O.nx, P.out.nx, w)); HIPCK(down(O.ny, P.out.ny, w)); HIPCK(down(O.nz, P.out.nz, w));
    HIPCK(down(O.cov9, P.out.cov9, 9 * w)); HIPCK(down(O.idx, P.out.idx, w));
  }
  HIPCK(hipStreamSynchronize(s));
  for (int q = 0; q < 3 && E.on; ++q)
    if (hipEventElapsedTime(&g_downsample_ms[q], E.ev[q], E.ev[q + 1]) != hipSuccess) g_downsample_ms[q] = 0.f;
  *n_out = total;
  return FDM_OK;
}
}  // namespace

namespace fdmh {
bool cloud_profile_on() { return g_downsample_profile; }
}  // namespace fdmh

extern "C" {

int fdm_cloud_voxel_grid(uint64_t n, const fdm_cloud_view* in, int on_device, float voxel_size, int mode, int order,
                         int device, const fdm_cloud_out* out, uint64_t* n_out) {
  if (mode < kVxCentroid || mode > kVxCenter) {
    if (n_out) *n_out = 0;
    return fail(FDM_ERR_INVALID, "mode must be 0 (CENTROID), 1 (NEAREST), 2 (ANY) or 3 (CENTER)");
  }
  return cloud_downsample(n, in, on_device, voxel_size, mode, order, device, out, n_out);
}

int fdm_cloud_grid_max_z(uint64_t n, const fdm_cloud_view* in, int on_device, float grid_size, int order, int device,
                         const fdm_cloud_out* out, uint64_t* n_out) {
  return cloud_downsample(n, in, on_device, grid_size, kVxMaxZ, order, device, out, n_out);
}

int fdm_cloud_debug_profile(int on) {
  g_downsample_profile = on != 0;
  g_downsample_ms[0] = g_downsample_ms[1] = g_downsample_ms[2] = 0.f;
  return FDM_OK;
}

int fdm_cloud_debug_last_ms(float ms3[3]) {
  if (!ms3) return fail(FDM_ERR_INVALID, "null argument");
  for (int q = 0; q < 3; ++q) ms3[q] = g_downsample_ms[q];
  return FDM_OK;
}

}  // extern "C"
