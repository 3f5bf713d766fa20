// fdm_engine_normals.inl — host side of normal and covariance estimation (kernels: fdm_normals.hpp): entry points
// fdm_cloud_estimate_normals and fdm_normals_last_stats.  Part of fdm_engine_post.hip, behind fdm_engine_dem.inl, whose
// search grid it builds (knn_grid_build) and whose bucket rule it dispatches by.  A cloud has no map and no engine: the
// call picks its device, works on the null stream in scratch of its own and frees it on return.  Synchronous.

namespace {
thread_local fdm_normal_stats g_normal_stats = {};

// five device events around the four stages, created only while fdm_cloud_debug_profile is on
struct NrmClock {
  hipEvent_t ev[5] = {};
  bool on = false;
  ~NrmClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
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

// effective_k = min(size_t(k), n) (kdtree_impl.hpp:76-94): a negative int converts to a huge size_t
uint64_t normals_effective_k(uint64_t n, int k) { return k < 0 ? n : std::min<uint64_t>(uint64_t(k), n); }

template <int KB>
void nrm_search(hipStream_t s, unsigned n, int k, const KnnIndex& I, const float* dx, const float* dy, const float* dz,
                const NrmOut& O) {
  hipLaunchKernelGGL((k_nrm_search<KB>), dim3((n + 255u) / 256u), dim3(256), 0, s, n, k, I.pts(), I.start(), I.G, dx, dy,
                     dz, O, I.queue(), I.st());
}
template <int KB>
void nrm_brute(hipStream_t s, unsigned nq, unsigned n, int k, const KnnIndex& I, const float* dx, const float* dy,
               const float* dz, const NrmOut& O) {
  hipLaunchKernelGGL((k_nrm_brute<KB>), dim3(nq), dim3(kNrmBruteThreads), 0, s, I.queue(), n, k, I.pts(), dx, dy, dz, O,
                     I.st());
}

// n device points, 3 <= k <= min(64, n): O's arrays are filled, *n_invalid set.  Marks E[0 .. 3]; synchronous on s.
int normals_device(hipStream_t s, unsigned n, const float* dx, const float* dy, const float* dz, int k, const NrmOut& O,
                   NrmClock& E, uint64_t* n_invalid) {
  if (int rc = E.mark(0, s)) return rc;
  KnnIndex I;
  if (int rc = knn_grid_build(s, n, dx, dy, dz, unsigned(k), I)) return rc;
  g_normal_stats.grid_x = I.G.gx;
  g_normal_stats.grid_y = I.G.gy;
  g_normal_stats.voxel = I.G.h;
  if (int rc = E.mark(1, s)) return rc;
  const int bucket = knn_bucket(k);
  switch (bucket) {
    case 4: nrm_search<4>(s, n, k, I, dx, dy, dz, O); break;
    case 16: nrm_search<16>(s, n, k, I, dx, dy, dz, O); break;
    case 32: nrm_search<32>(s, n, k, I, dx, dy, dz, O); break;
    default: nrm_search<64>(s, n, k, I, dx, dy, dz, O); break;
  }
  HIPCK(hipGetLastError());
  if (int rc = E.mark(2, s)) return rc;
  KnnStat hs{};
  HIPCK(hipMemcpyAsync(&hs, I.st(), sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  const unsigned nq = hs.n_queue;
  if (nq > n) return fail(FDM_ERR_HIP, "k-NN queue overran the cloud");
  g_normal_stats.n_fallback = nq;
  if (nq) {
    switch (bucket) {
      case 4: nrm_brute<4>(s, nq, n, k, I, dx, dy, dz, O); break;
      case 16: nrm_brute<16>(s, nq, n, k, I, dx, dy, dz, O); break;
      case 32: nrm_brute<32>(s, nq, n, k, I, dx, dy, dz, O); break;
      default: nrm_brute<64>(s, nq, n, k, I, dx, dy, dz, O); break;
    }
    HIPCK(hipGetLastError());
  }
  if (int rc = E.mark(3, s)) return rc;
  HIPCK(hipMemcpyAsync(&hs, I.st(), sizeof(hs), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (hs.n_invalid > n) return fail(FDM_ERR_HIP, "the invalid count overran the cloud");
  *n_invalid = hs.n_invalid;
  return FDM_OK;
}
}  // namespace

extern "C" {

int fdm_normals_last_stats(fdm_normal_stats* out) {
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  *out = g_normal_stats;
  return FDM_OK;
}

int fdm_cloud_estimate_normals(uint64_t n, const float* x, const float* y, const float* z, int on_device, int k,
                               const float viewpoint[3], int device, float* nx, float* ny, float* nz, float* cov9,
                               uint64_t* n_invalid) {
  if (n_invalid) *n_invalid = 0;
  g_normal_stats = fdm_normal_stats{};
  const int normals = int(nx != nullptr) + int(ny != nullptr) + int(nz != nullptr);
  if (normals != 0 && normals != 3) return fail(FDM_ERR_INVALID, "normals need all of nx, ny, nz");
  if (normals == 0 && !cov9) return fail(FDM_ERR_INVALID, "nothing to estimate: give nx, ny, nz or cov9");
  if (int rc = check_cloud(n, x, y, z)) return rc;
  const uint64_t k_eff = normals_effective_k(n, k);
  if (k_eff > uint64_t(kKnnMaxK)) return fail(FDM_ERR_INVALID, "normal estimation takes at most 64 neighbours");
  if (n == 0) return FDM_OK;
  const ScopedDevice restore;
  if (int rc = pick_device(device)) return rc;
  hipStream_t s = nullptr;
  const unsigned np = unsigned(n);
  const bool host = on_device == 0;
  NrmClock E;
  if (int rc = E.init(cloud_profile_on())) return rc;

  CloudBlock b_in, b_out;  // a host cloud's coordinates, and its outputs: nx, ny, nz, then cov9
  const void* const src[3] = {x, y, z};
  const float* d[3];
  if (int rc = stage_cloud(s, n, 3, src, !host, b_in, d)) return rc;
  NrmOut O{nx, ny, nz, cov9, 0.0f, 0.0f, 0.0f};
  if (viewpoint) { O.vx = viewpoint[0]; O.vy = viewpoint[1]; O.vz = viewpoint[2]; }
  if (host) {
    if (int rc = b_out.alloc(size_t(n), (normals ? 3 : 0) + (cov9 ? 9 : 0))) return rc;
    O.nx = normals ? b_out.ch(0) : nullptr;
    O.ny = normals ? b_out.ch(1) : nullptr;
    O.nz = normals ? b_out.ch(2) : nullptr;
    O.cov9 = cov9 ? b_out.ch(normals ? 3 : 0) : nullptr;
  }
  g_normal_stats.n_queries = n;
  uint64_t bad = 0;
  if (k_eff < uint64_t(kNrmMinNeighbors)) {  // fewer than MIN_NEIGHBORS: every point invalid, nothing is searched
    hipLaunchKernelGGL(k_nrm_invalid, dim3((np + 255u) / 256u), dim3(256), 0, s, np, O);
    HIPCK(hipGetLastError());
    bad = n;
    for (int q = 0; q < 4; ++q)
      if (int rc = E.mark(q, s)) return rc;
  } else if (int rc = normals_device(s, np, d[0], d[1], d[2], int(k_eff), O, E, &bad)) {
    return rc;
  }
  if (host) {
    const size_t w = size_t(n) * sizeof(float);
    if (normals) {
      HIPCK(hipMemcpyAsync(nx, O.nx, w, hipMemcpyDeviceToHost, s));
      HIPCK(hipMemcpyAsync(ny, O.ny, w, hipMemcpyDeviceToHost, s));
      HIPCK(hipMemcpyAsync(nz, O.nz, w, hipMemcpyDeviceToHost, s));
    }
    if (cov9) HIPCK(hipMemcpyAsync(cov9, O.cov9, 9 * w, hipMemcpyDeviceToHost, s));
  }
  if (int rc = E.mark(4, s)) return rc;
  HIPCK(hipStreamSynchronize(s));
  for (int q = 0; q < 4 && E.on; ++q)
    if (hipEventElapsedTime(&g_normal_stats.ms[q], E.ev[q], E.ev[q + 1]) != hipSuccess) g_normal_stats.ms[q] = 0.f;
  g_normal_stats.n_invalid = bad;
  if (n_invalid) *n_invalid = bad;
  return FDM_OK;
}

}  // extern "C"
