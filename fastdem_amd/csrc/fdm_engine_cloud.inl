// fdm_engine_cloud.inl — what the host files of the cloud and file stages share: scoped device scratch, the layout of a
// cloud's channels in one device block and their upload, the argument checks with their messages, the map over a cloud's
// bounding box, the per-block counters of the pack / compact kernels.  The head of fdm_engine_post.hip: the .inl files
// behind it (io, raster, dem, pcd) use it.  (The radix sort's driver is in fdm_rsort.hpp, which the ray unit shares; the
// device check and grow_device are fdmh's, fdm_engine.hip.)

namespace {
constexpr uint64_t kRasMaxPoints = 1ull << 31;

struct DevBuf {  // a device allocation that lives as long as its scope
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) {
    HIPCK(hipMalloc(&p, bytes ? bytes : 4));
    return FDM_OK;
  }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};
struct Events {
  hipEvent_t ev[12] = {};
  ~Events() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
  int init(int count) {
    for (int k = 0; k < count; ++k) HIPCK(hipEventCreate(&ev[k]));
    return FDM_OK;
  }
  float ms(int a, int b) const {
    float t = 0.f;
    return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? t : 0.f;
  }
};

float unord_host(uint32_t u) {  // the host's image of the device's unord(): the float an ordered key stands for
  const uint32_t b = u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu);
  float f;
  std::memcpy(&f, &b, sizeof(f));
  return f;
}

// ---- a cloud's channels in ONE device block: channel k of n points at base + k * cloud_stride(n), a multiple of four
// points, so that every channel starts 16-byte aligned (as in StageSlot) ----
size_t cloud_stride(size_t n) { return (n + 3) & ~size_t(3); }
// ... of an engine-owned block for n points that is kept for the next call: a quarter and 1 024 points of slack
size_t cloud_cap(size_t n) { return cloud_stride(n + n / 4 + 1024); }
struct CloudBlock {  // a block of the call's own
  DevBuf mem;
  size_t stride = 0;
  int alloc(size_t n, int count) {
    stride = cloud_stride(n);
    return mem.alloc(stride * size_t(count) * sizeof(float));
  }
  float* ch(int k) const { return mem.as<float>() + stride * size_t(k); }
};
// the present ones (non-null) of `count` host channels into the block at `base`, on stream s; dev[k] = where channel k is
// on the device, null for an absent one.  Enqueue-only: the copies read the caller's arrays until s has drained.  Every
// entry that uses this synchronises s before it returns FDM_OK; where it returns an error first, the block's hipFree
// (~DevBuf, which waits for the device) is what ends the copies before the caller has its arrays back.  (The engine-
// owned block of fdm_engine_from_point_cloud is not freed: an error return there, as ever, does not wait.)
template <typename P>
int upload_cloud(hipStream_t s, uint64_t n, int count, const void* const* host, float* base, size_t stride, P* dev) {
  for (int k = 0; k < count; ++k) {
    dev[k] = nullptr;
    if (!host[k]) continue;
    float* const d = base + stride * size_t(k);
    HIPCK(hipMemcpyAsync(d, host[k], size_t(n) * sizeof(float), hipMemcpyHostToDevice, s));
    dev[k] = d;
  }
  return FDM_OK;
}
// ... of a cloud the caller says is on the host or on the device already: B is allocated only for a host cloud
template <typename P>
int stage_cloud(hipStream_t s, uint64_t n, int count, const void* const* src, bool on_device, CloudBlock& B, P* dev) {
  if (on_device) {
    for (int k = 0; k < count; ++k) dev[k] = static_cast<P>(src[k]);
    return FDM_OK;
  }
  if (int rc = B.alloc(size_t(n), count)) return rc;
  return upload_cloud(s, n, count, src, B.ch(0), B.stride, dev);
}

// ---- argument checks (callers and tests read the texts) ----
// a cloud of n points with x, y, z [and the rasterization method it is meant for]
int check_cloud(uint64_t n, const void* x, const void* y, const void* z, int method = 0) {
  if (n >= kRasMaxPoints) return fail(FDM_ERR_INVALID, "point count exceeds 2^31-1");
  if (method < 0 || method > 3) return fail(FDM_ERR_INVALID, "method must be 0 (Max), 1 (Min), 2 (Mean) or 3 (MinMax)");
  if (n && (!x || !y || !z)) return fail(FDM_ERR_INVALID, "null coordinate array");
  return FDM_OK;
}
int check_resolution(float resolution) {
  if (!(resolution > 0.0f) || !std::isfinite(resolution)) return fail(FDM_ERR_INVALID, "resolution must be positive");
  return FDM_OK;
}

// An empty map over the x / y bounding box of n device points (pcd_convert.cpp:155-181, :285-305); `device` is current.
// Synchronous, on the null stream: the map does not exist yet.
int map_over_cloud(unsigned n, const float* dx, const float* dy, float resolution, int device, fdm_engine** out) {
  *out = nullptr;
  DevBuf b_stat;
  if (int rc = b_stat.alloc(sizeof(RasterStat))) return rc;
  hipLaunchKernelGGL(k_ras_stat_init, dim3(1), dim3(64), 0, nullptr, b_stat.as<RasterStat>());
  hipLaunchKernelGGL(k_ras_bounds, dim3(std::min((n + 255u) / 256u, 2048u)), dim3(256), 0, nullptr, n, dx, dy,
                     b_stat.as<RasterStat>());
  HIPCK(hipGetLastError());
  RasterStat hs{};
  HIPCK(hipMemcpy(&hs, b_stat.p, sizeof(hs), hipMemcpyDeviceToHost));
  const float min_x = unord_host(hs.min_x), min_y = unord_host(hs.min_y);
  const float max_x = unord_host(hs.max_x), max_y = unord_host(hs.max_y);
  // one cell of margin (:175-176), in fp32 as the reference computes it
  const float width = max_x - min_x + resolution, height = max_y - min_y + resolution;
  // an extent that is not a positive finite number (no point with both coordinates, an infinite coordinate) is
  // undefined behaviour in the reference (a map of no or of 2^31 cells): refused here
  if (!std::isfinite(width) || !std::isfinite(height) || !(width > 0.0f) || !(height > 0.0f))
    return fail(FDM_ERR_INVALID, "the cloud's x / y extent is not a positive finite number");
  fdm_geometry g{};
  g.length_x = double(width);  // ElevationMap::setGeometry(float, float, float): promoted
  g.length_y = double(height);
  g.resolution = double(resolution);
  g.position_x = double(min_x + max_x) / 2.0;  // an fp32 sum, an fp64 divide (:180-181)
  g.position_y = double(min_y + max_y) / 2.0;
  const int rc = fdm_engine_create_map(&g, nullptr, device, out);
  if (rc) *out = nullptr;
  return rc;
}

// per-block counts / offsets of the count-scan-write kernels (ingest, egress, toPointCloud): blocks + 1 words
int ensure_pack_counts(fdm_engine* e, unsigned blocks) {
  const size_t need = size_t(blocks) + 1;
  return grow_device(e, &e->pack_counts, &e->pack_counts_cap, need, need + 1024);
}
}  // namespace
