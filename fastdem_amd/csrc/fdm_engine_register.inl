// fdm_engine_register.inl — host side of cloud registration (kernels: fdm_register.hpp, fdm_vgicp.hpp; the 6 x 6 algebra
// and the loop: fdm_register_host.hpp): ONE path behind ICP, plane ICP, GICP and voxelized GICP.  A RegProblem states the
// method, the source, the target — the target fields of fdm_register_clouds, or a voxel map — and the device; reg_check
// refuses what is refused before a device is touched, RegCall::prepare stages the source, sets the target up and
// regularises the covariances, and reg_align / reg_linearize hold everything else an entry does.  The entry points here
// (fdm_cloud_register, fdm_cloud_register_linearize) and in fdm_engine_vgicp.inl (the two _vgicp entries) pack their
// arguments and make one call.  Also fdm_register_last_stats and fdm_default_align_settings.
// Part of fdm_engine_post.hip, behind fdm_engine_normals.inl; the target's search grid is fdm_engine_dem.inl's
// (knn_grid_build).  Engine-free like the other cloud calls: the call picks its device, works on the null stream in
// scratch of its own and frees it on return.  Synchronous: the host reads 29 doubles per iteration.

// The voxel distribution map (built, owned and handed out by fdm_engine_vgicp.inl), stated here because a registration
// against it reads its device, its voxel count and its table.
struct fdm_voxel_map {
  fdm_voxel_map_info info{};
  void* rec_mem = nullptr;    // the records, one block
  void* table_mem = nullptr;  // slot keys, then slot ranks
  VgRecords R{};
  VgTable T{};
};

namespace {
thread_local fdm_register_stats g_register_stats = {};

// The ring limit of the walk: the first ring whose stopping bound — taken at margin 0, the smallest it can be, by the
// device's own arithmetic (knn_walk) — already excludes everything within the radius, capped by the ring that holds the
// whole grid from any column.  Every lane therefore leaves the walk by one of its exits; nothing is queued.
int reg_ring_limit(const KnnGrid& G, float max_d2) {
  const int cap = std::max(G.gx, G.gy) - 1;
  for (int s = 0; s < cap; ++s) {
    const float lb = ((float(s) - 0.00390625f) * G.h) * 0.9999f;
    if (lb > 0.0f && max_d2 < (lb * lb) * 0.9999f) return s;
  }
  return cap;
}

// One registration problem, as an entry point states it.
struct RegProblem {
  int method = kRegICP;
  uint64_t n = 0;  // the source
  const float *x = nullptr, *y = nullptr, *z = nullptr, *cov9 = nullptr;
  bool on_device = false;
  bool voxels = false;                          // the target is `map` (then method = kRegVGICP), else the t* fields of `clouds`
  const fdm_register_clouds* clouds = nullptr;
  const fdm_voxel_map* map = nullptr;
  int device = 0;                               // where the call runs: the caller's choice, or the map's device
  uint64_t n_target() const { return voxels ? map->info.num_voxels : clouds->n_target; }
};

struct RegCall {
  int method = 0;
  unsigned n_src = 0, n_tgt = 0;
  fdm_align_settings set{};
  hipStream_t s = nullptr;
  CloudBlock b_src, b_tgt;
  DevBuf b_scov, b_tcov, b_screg, b_tcreg, b_partial, b_out, b_corr, b_stat;
  KnnIndex I;
  const float* src[3] = {};
  const float* tgt[6] = {};
  RegTarget Q{};
  VgTable V{};  // kRegVGICP: the map's table and records
  Events E;
  bool clock = false;
  int32_t* d_corr = nullptr;

  int mark(int k) {
    if (clock) HIPCK(hipEventRecord(E.ev[k], s));
    return FDM_OK;
  }
  // the source on the device, and the refusal of a coordinate that is not finite: it has no grid of its own, its
  // coordinates are looked at by the bounds kernel alone
  int stage_source(const RegProblem& P) {
    clock = cloud_profile_on();
    if (clock)
      if (int rc = E.init(6)) return rc;
    const void* const h_src[3] = {P.x, P.y, P.z};
    if (int rc = stage_cloud(s, P.n, 3, h_src, P.on_device, b_src, src)) return rc;
    if (int rc = b_stat.alloc(sizeof(KnnStat))) return rc;
    hipLaunchKernelGGL(k_knn_init, dim3(1), dim3(64), 0, s, b_stat.as<KnnStat>());
    hipLaunchKernelGGL(k_knn_bounds, dim3(std::min((n_src + 255u) / 256u, 2048u)), dim3(256), 0, s, n_src, src[0], src[1],
                       src[2], b_stat.as<KnnStat>());
    HIPCK(hipGetLastError());
    KnnStat hs{};
    HIPCK(hipMemcpyAsync(&hs, b_stat.p, sizeof(hs), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (hs.nonfinite) return fail(FDM_ERR_INVALID, "the source cloud has a coordinate that is not finite");
    return FDM_OK;
  }
  // a target cloud: staging, its search grid (which refuses a coordinate that is not finite), what the walk reads
  int target_cloud(const fdm_register_clouds& c, bool dev) {
    n_tgt = unsigned(c.n_target);
    const void* const ht[6] = {c.tx, c.ty, c.tz, method == kRegPlane ? c.tnx : nullptr, method == kRegPlane ? c.tny : nullptr,
                               method == kRegPlane ? c.tnz : nullptr};
    if (int rc = stage_cloud(s, c.n_target, 6, ht, dev, b_tgt, tgt)) return rc;
    if (int rc = mark(0)) return rc;
    if (int rc = knn_grid_build(s, n_tgt, tgt[0], tgt[1], tgt[2], 1u, I)) return rc;
    if (int rc = mark(1)) return rc;
    const float max_d2 = set.max_correspondence_dist * set.max_correspondence_dist;
    Q.pts = I.pts();
    Q.start = I.start();
    Q.G = I.G;
    Q.rings = reg_ring_limit(I.G, max_d2);
    Q.max_d2 = max_d2;
    Q.n = n_tgt;
    Q.x = tgt[0]; Q.y = tgt[1]; Q.z = tgt[2];
    Q.nx = tgt[3]; Q.ny = tgt[4]; Q.nz = tgt[5];
    g_register_stats.n_source = n_src;
    g_register_stats.n_target = n_tgt;
    g_register_stats.grid_x = I.G.gx;
    g_register_stats.grid_y = I.G.gy;
    g_register_stats.voxel = I.G.h;
    g_register_stats.ring_limit = Q.rings;
    return FDM_OK;
  }
  // a voxel map, built elsewhere: its table (no grid, no rings: those statistics stay 0)
  int target_map(const fdm_voxel_map& m) {
    n_tgt = unsigned(std::min<uint64_t>(m.info.num_voxels, 0xFFFFFFFFull));
    V = m.T;
    g_register_stats.n_source = n_src;
    g_register_stats.n_target = m.info.num_voxels;
    g_register_stats.voxel = m.info.resolution;
    return FDM_OK;
  }
  // a cloud's covariances (9 floats per point; staged in `stage` when they are the host's) regularised into `creg`
  int regularize(const float* cov9, unsigned n, bool dev, DevBuf& stage, DevBuf& creg) {
    if (!dev) {
      if (int rc = stage.alloc(size_t(n) * 9 * sizeof(float))) return rc;
      HIPCK(hipMemcpyAsync(stage.p, cov9, size_t(n) * 9 * sizeof(float), hipMemcpyHostToDevice, s));
      cov9 = stage.as<float>();
    }
    if (int rc = creg.alloc(size_t(n) * 6 * sizeof(double))) return rc;
    hipLaunchKernelGGL(k_reg_regularize, dim3((n + 255u) / 256u), dim3(256), 0, s, n, cov9, set.covariance_epsilon,
                       creg.as<double>());
    HIPCK(hipGetLastError());
    return FDM_OK;
  }
  // a problem that passed reg_check and is not empty, its device current: everything a linearization reads
  int prepare(const RegProblem& P, const fdm_align_settings& st) {
    method = P.method;
    set = st;
    n_src = unsigned(P.n);
    if (P.voxels && P.on_device) {  // device arrays are the caller's: they must live where the map does (asked before
      hipPointerAttribute_t at{};   // a kernel reads them)
      if (hipPointerGetAttributes(&at, P.x) != hipSuccess)
        (void)hipGetLastError();  // (not a pointer the runtime knows: left to the copy that reads it)
      else if (at.type == hipMemoryTypeDevice && at.device != P.map->info.device)
        return fail(FDM_ERR_INVALID, "the voxel map was built on another device than the source lives on");
    }
    if (int rc = stage_source(P)) return rc;
    if (int rc = P.voxels ? target_map(*P.map) : target_cloud(*P.clouds, P.on_device)) return rc;
    if (int rc = mark(2)) return rc;
    if (method == kRegGICP || method == kRegVGICP)
      if (int rc = regularize(P.cov9, n_src, P.on_device, b_scov, b_screg)) return rc;
    if (method == kRegGICP) {
      if (int rc = regularize(P.clouds->t_cov9, n_tgt, P.on_device, b_tcov, b_tcreg)) return rc;
      Q.creg = b_tcreg.as<double>();
    }
    if (int rc = mark(3)) return rc;
    // one partial per block of the linearization, and their sum
    const unsigned blocks = (n_src + unsigned(kRegThreads) - 1u) / unsigned(kRegThreads);
    if (int rc = b_partial.alloc(size_t(blocks) * kRegStride * sizeof(double))) return rc;
    return b_out.alloc(kRegStride * sizeof(double));
  }
  // one linearization at T: the model, and the correspondences where d_corr is set
  int linearize(const reg::Rigid& T, reg::Model& M) {
    RegTransform t;
    for (int r = 0; r < 3; ++r) {
      for (int q = 0; q < 3; ++q) t.r[r * 3 + q] = T.R[r][q];
      t.t[r] = T.t[r];
    }
    const unsigned blocks = (n_src + unsigned(kRegThreads) - 1u) / unsigned(kRegThreads);
    double* const part = b_partial.as<double>();
    const int kern = method == kRegICP ? int(kRegNone) : set.robust_kernel;
    const double width = set.robust_kernel_width;
    const double* const none = nullptr;
    const double* const screg = b_screg.as<double>();
    if (int rc = mark(4)) return rc;
    switch (method) {
      case kRegICP:
        hipLaunchKernelGGL((k_reg_linearize<kRegICP>), dim3(blocks), dim3(kRegThreads), 0, s, n_src, src[0], src[1], src[2],
                           none, t, Q, kern, width, part, d_corr);
        break;
      case kRegPlane:
        hipLaunchKernelGGL((k_reg_linearize<kRegPlane>), dim3(blocks), dim3(kRegThreads), 0, s, n_src, src[0], src[1], src[2],
                           none, t, Q, kern, width, part, d_corr);
        break;
      case kRegGICP:
        hipLaunchKernelGGL((k_reg_linearize<kRegGICP>), dim3(blocks), dim3(kRegThreads), 0, s, n_src, src[0], src[1], src[2],
                           screg, t, Q, kern, width, part, d_corr);
        break;
      case kRegVGICP:
        hipLaunchKernelGGL(k_vg_linearize, dim3(blocks), dim3(kRegThreads), 0, s, n_src, src[0], src[1], src[2], screg, t,
                           V, kern, width, part, d_corr);
        break;
    }
    hipLaunchKernelGGL(k_reg_reduce, dim3(1), dim3(kRegSlices * kRegStride), 0, s, blocks, part, b_out.as<double>());
    HIPCK(hipGetLastError());
    if (int rc = mark(5)) return rc;
    double h[kRegSums];
    HIPCK(hipMemcpyAsync(h, b_out.p, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    for (int a = 0; a < 21; ++a) M.H[a] = h[a];
    for (int a = 0; a < 6; ++a) M.b[a] = h[21 + a];
    M.error = h[27];
    M.num_inliers = uint64_t(h[28]);
    g_register_stats.linearizations += 1;
    if (clock) g_register_stats.ms[2] += E.ms(4, 5);
    return FDM_OK;
  }
  void finish() {
    if (!clock) return;
    if (method != kRegVGICP) g_register_stats.ms[0] = E.ms(0, 1);  // (a voxel map was built elsewhere)
    g_register_stats.ms[1] = E.ms(2, 3);
  }
};

// what every entry refuses before a device is touched, in the order callers and tests rely on; *empty: the reference's
// early return applies (and nothing behind it is looked at)
int reg_check(const RegProblem& P, const double* T16, const fdm_align_settings& st, bool* empty) {
  *empty = false;
  if (P.voxels ? !P.map : !P.clouds) return fail(FDM_ERR_INVALID, "null argument");
  if (!P.voxels && (P.method < kRegICP || P.method > kRegGICP))
    return fail(FDM_ERR_INVALID, "method must be 0 (ICP), 1 (PLANE) or 2 (GICP)");
  if (st.robust_kernel < kRegNone || st.robust_kernel > kRegCauchy)
    return fail(FDM_ERR_INVALID, "robust_kernel must be 0 (NONE), 1 (HUBER), 2 (TUKEY) or 3 (CAUCHY)");
  if (!P.voxels && !(st.max_correspondence_dist >= 0.0f))  // (voxelized GICP does not use it)
    return fail(FDM_ERR_INVALID, "max_correspondence_dist must not be negative or NaN");
  if (T16)
    for (int a = 0; a < 16; ++a)
      if (!std::isfinite(T16[a])) return fail(FDM_ERR_INVALID, "the transform has an entry that is not finite");
  if (int rc = check_cloud(P.n, P.x, P.y, P.z)) return rc;
  if (!P.voxels)
    if (int rc = check_cloud(P.clouds->n_target, P.clouds->tx, P.clouds->ty, P.clouds->tz)) return rc;
  if (P.n == 0 || P.n_target() == 0) {
    *empty = true;
    return FDM_OK;
  }
  if (P.method == kRegPlane && (!P.clouds->tnx || !P.clouds->tny || !P.clouds->tnz))
    return fail(FDM_ERR_INVALID, "alignPlaneICP: target must have normals (all of nx, ny, nz)");
  if (P.method == kRegGICP && !P.cov9) return fail(FDM_ERR_INVALID, "alignGICP: source must have covariances");
  if (P.method == kRegGICP && !P.clouds->t_cov9) return fail(FDM_ERR_INVALID, "alignGICP: target must have covariances");
  if (P.method == kRegVGICP && !P.cov9) return fail(FDM_ERR_INVALID, "alignVGICP: source must have covariances");
  return FDM_OK;
}
fdm_align_settings reg_settings(const fdm_align_settings* st) {
  fdm_align_settings d;
  fdm_default_align_settings(&d);
  return st ? *st : d;
}
reg::Rigid reg_rigid(const double* T16) { return T16 ? reg::rigid_from_colmajor(T16) : reg::rigid_identity(); }
// the host loop over call.linearize, from `guess`
int reg_solve(RegCall& call, uint64_t n_source, const reg::Rigid& guess, const fdm_align_settings& st, reg::Result* R) {
  reg::Criteria crit;
  crit.max_iterations = st.max_iterations;
  crit.min_correspondences = st.min_correspondences;
  crit.translation_eps = st.translation_eps;
  crit.rotation_eps = st.rotation_eps;
  crit.relative_error_eps = st.relative_error_eps;
  int rc = FDM_OK;
  *R = reg::solve(n_source, guess, crit, [&](const reg::Rigid& T, reg::Model& M) { return call.linearize(T, M); }, &rc);
  if (rc) return rc;
  call.finish();
  return FDM_OK;
}
void reg_write_result(const reg::Result& R, fdm_registration_result* out) {
  *out = fdm_registration_result{};
  reg::rigid_to_colmajor(R.T, out->transform);
  out->fitness = R.fitness;
  out->rmse = R.rmse;
  out->iterations = R.iterations;
  out->converged = R.converged ? 1 : 0;
  out->has_covariance = R.has_covariance ? 1 : 0;
  if (R.has_covariance) std::memcpy(out->covariance, R.covariance, sizeof(out->covariance));
}

// The two drivers: what an entry does once its arguments are a RegProblem.
int reg_align(const RegProblem& P, const double* initial_guess, const fdm_align_settings* settings,
              fdm_registration_result* out) {
  g_register_stats = fdm_register_stats{};
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  const fdm_align_settings st = reg_settings(settings);
  bool empty = false;
  if (int rc = reg_check(P, initial_guess, st, &empty)) return rc;
  const reg::Rigid guess = reg_rigid(initial_guess);
  reg::Result R = reg::failed_result(guess, 0);  // the early return of an empty source or target (align.hpp:76-78, :281-283)
  if (!empty) {
    const ScopedDevice restore;
    if (int rc = pick_device(P.device)) return rc;
    RegCall call;
    if (int rc = call.prepare(P, st)) return rc;
    if (int rc = reg_solve(call, P.n, guess, st, &R)) return rc;
  }
  reg_write_result(R, out);
  return FDM_OK;
}
int reg_linearize(const RegProblem& P, const double* transform, const fdm_align_settings* settings, double H[21],
                  double b[6], double* error, uint64_t* num_inliers, int32_t* corr) {
  g_register_stats = fdm_register_stats{};
  if (!H || !b || !error || !num_inliers) return fail(FDM_ERR_INVALID, "null argument");
  const fdm_align_settings st = reg_settings(settings);
  bool empty = false;
  if (int rc = reg_check(P, transform, st, &empty)) return rc;
  reg::Model M;
  const size_t corr_bytes = size_t(P.n) * sizeof(int32_t);
  if (!empty) {
    const ScopedDevice restore;
    if (int rc = pick_device(P.device)) return rc;
    RegCall call;
    if (int rc = call.prepare(P, st)) return rc;
    call.d_corr = corr;
    if (corr && !P.on_device) {  // a host caller's: written on the device, then downloaded
      if (int rc = call.b_corr.alloc(corr_bytes)) return rc;
      call.d_corr = call.b_corr.as<int32_t>();
    }
    if (int rc = call.linearize(reg_rigid(transform), M)) return rc;
    if (corr && !P.on_device) HIPCK(hipMemcpy(corr, call.d_corr, corr_bytes, hipMemcpyDeviceToHost));
    call.finish();
  } else if (corr && P.n) {  // no target: nobody corresponds
    if (P.on_device) {
      const ScopedDevice restore;
      if (int rc = pick_device(P.device)) return rc;
      HIPCK(hipMemset(corr, 0xFF, corr_bytes));
    } else {
      std::memset(corr, 0xFF, corr_bytes);
    }
  }
  std::memcpy(H, M.H, sizeof(M.H));
  std::memcpy(b, M.b, sizeof(M.b));
  *error = M.error;
  *num_inliers = M.num_inliers;
  return FDM_OK;
}
RegProblem reg_problem(int method, const fdm_register_clouds* c, int device) {
  RegProblem P;
  P.method = method;
  P.clouds = c;
  P.device = device;
  if (c) {
    P.n = c->n_source;
    P.x = c->sx; P.y = c->sy; P.z = c->sz;
    P.cov9 = c->s_cov9;
    P.on_device = c->on_device != 0;
  }
  return P;
}
}  // namespace

extern "C" {

void fdm_default_align_settings(fdm_align_settings* s) {  // AlignSettings{} (align.hpp:32-59)
  if (!s) return;
  *s = fdm_align_settings{};
  s->max_correspondence_dist = 1.0f;
  s->max_iterations = 50;
  s->translation_eps = 1e-4;
  s->rotation_eps = 1e-4;
  s->relative_error_eps = 1e-6;
  s->min_correspondences = 10;
  s->robust_kernel = kRegNone;
  s->robust_kernel_width = 1.0;
  s->covariance_epsilon = 1e-3;
}

int fdm_register_last_stats(fdm_register_stats* out) {
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  *out = g_register_stats;
  return FDM_OK;
}

int fdm_cloud_register(int method, const fdm_register_clouds* clouds, const double* initial_guess,
                       const fdm_align_settings* settings, int device, fdm_registration_result* out) {
  return reg_align(reg_problem(method, clouds, device), initial_guess, settings, out);
}

int fdm_cloud_register_linearize(int method, const fdm_register_clouds* clouds, const double* transform,
                                 const fdm_align_settings* settings, int device, double H[21], double b[6], double* error,
                                 uint64_t* num_inliers, int32_t* corr) {
  return reg_linearize(reg_problem(method, clouds, device), transform, settings, H, b, error, num_inliers, corr);
}

}  // extern "C"
