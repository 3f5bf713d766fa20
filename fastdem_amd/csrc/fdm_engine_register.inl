// fdm_engine_register.inl — host side of cloud registration (kernels: fdm_register.hpp; the 6 x 6 algebra and the loop:
// fdm_register_host.hpp): entry points fdm_cloud_register, fdm_cloud_register_linearize, fdm_register_last_stats and
// fdm_default_align_settings.  Part of fdm_engine_post.hip, behind fdm_engine_normals.inl; the target's search grid is
// fdm_engine_dem.inl's (knn_grid_build).  Engine-free like the other cloud calls: the call picks its device, works on the
// null stream in scratch of its own and frees it on return.  Synchronous: the host reads 29 doubles per iteration.
// RegCall's steps (the source's staging and finite check, its regularisation, the partials) and reg_solve also serve
// voxelized GICP, whose target is a prebuilt voxel map (fdm_engine_vgicp.inl).

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
  VgTable V{};  // kRegVGICP: the map's table and records (fdm_engine_vgicp.inl)
  Events E;
  bool clock = false;
  int32_t* d_corr = nullptr;

  int mark(int k) {
    if (clock) HIPCK(hipEventRecord(E.ev[k], s));
    return FDM_OK;
  }
  // a cloud's 9 floats per point, on the device
  int stage_cov(const float* cov9, uint64_t n, bool on_device, DevBuf& B, const float** d) {
    *d = cov9;
    if (on_device || !cov9) return FDM_OK;
    if (int rc = B.alloc(size_t(n) * 9 * sizeof(float))) return rc;
    HIPCK(hipMemcpyAsync(B.p, cov9, size_t(n) * 9 * sizeof(float), hipMemcpyHostToDevice, s));
    *d = B.as<float>();
    return FDM_OK;
  }
  // both clouds non-empty and checked: staging, the refusal of a coordinate that is not finite, the target's grid, the
  // regularised covariances
  // the source on the device, and the refusal of a coordinate that is not finite: it has no grid of its own, its
  // coordinates are looked at by the bounds kernel alone
  int stage_source(int method_, uint64_t n, const float* sx, const float* sy, const float* sz, bool dev,
                   const fdm_align_settings& st) {
    method = method_;
    set = st;
    n_src = unsigned(n);
    clock = cloud_profile_on();
    if (clock)
      if (int rc = E.init(6)) return rc;
    const void* const h_src[3] = {sx, sy, sz};
    if (int rc = stage_cloud(s, n, 3, h_src, dev, b_src, src)) return rc;
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
  // the source's regularised covariances
  int regularize_source(const float* s_cov9, bool dev) {
    const float* d_sc = nullptr;
    if (int rc = stage_cov(s_cov9, n_src, dev, b_scov, &d_sc)) return rc;
    if (int rc = b_screg.alloc(size_t(n_src) * 6 * sizeof(double))) return rc;
    hipLaunchKernelGGL(k_reg_regularize, dim3((n_src + 255u) / 256u), dim3(256), 0, s, n_src, d_sc, set.covariance_epsilon,
                       b_screg.as<double>());
    HIPCK(hipGetLastError());
    return FDM_OK;
  }
  // one partial per block of the linearization, and their sum
  int alloc_sums() {
    const unsigned blocks = (n_src + unsigned(kRegThreads) - 1u) / unsigned(kRegThreads);
    if (int rc = b_partial.alloc(size_t(blocks) * kRegStride * sizeof(double))) return rc;
    return b_out.alloc(kRegStride * sizeof(double));
  }
  int prepare(int method_, const fdm_register_clouds& c, const fdm_align_settings& st) {
    const bool dev = c.on_device != 0;
    if (int rc = stage_source(method_, c.n_source, c.sx, c.sy, c.sz, dev, st)) return rc;
    n_tgt = unsigned(c.n_target);
    const void* const ht[6] = {c.tx, c.ty, c.tz, method == kRegPlane ? c.tnx : nullptr, method == kRegPlane ? c.tny : nullptr,
                               method == kRegPlane ? c.tnz : nullptr};
    if (int rc = stage_cloud(s, c.n_target, 6, ht, dev, b_tgt, tgt)) return rc;
    if (int rc = mark(0)) return rc;
    if (int rc = knn_grid_build(s, n_tgt, tgt[0], tgt[1], tgt[2], 1u, I)) return rc;  // (refuses a target that is not finite)
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
    if (int rc = mark(2)) return rc;
    if (method == kRegGICP) {
      const float* d_tc = nullptr;
      if (int rc = regularize_source(c.s_cov9, dev)) return rc;
      if (int rc = stage_cov(c.t_cov9, c.n_target, dev, b_tcov, &d_tc)) return rc;
      if (int rc = b_tcreg.alloc(size_t(n_tgt) * 6 * sizeof(double))) return rc;
      hipLaunchKernelGGL(k_reg_regularize, dim3((n_tgt + 255u) / 256u), dim3(256), 0, s, n_tgt, d_tc, set.covariance_epsilon,
                         b_tcreg.as<double>());
      HIPCK(hipGetLastError());
      Q.creg = b_tcreg.as<double>();
    }
    if (int rc = mark(3)) return rc;
    return alloc_sums();
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
    if (int rc = mark(4)) return rc;
    switch (method) {
      case kRegICP:
        hipLaunchKernelGGL((k_reg_linearize<kRegICP>), dim3(blocks), dim3(kRegThreads), 0, s, n_src, src[0], src[1], src[2],
                           static_cast<const double*>(nullptr), t, Q, kern, width, part, d_corr);
        break;
      case kRegPlane:
        hipLaunchKernelGGL((k_reg_linearize<kRegPlane>), dim3(blocks), dim3(kRegThreads), 0, s, n_src, src[0], src[1], src[2],
                           static_cast<const double*>(nullptr), t, Q, kern, width, part, d_corr);
        break;
      case kRegVGICP:
        hipLaunchKernelGGL(k_vg_linearize, dim3(blocks), dim3(kRegThreads), 0, s, n_src, src[0], src[1], src[2],
                           static_cast<const double*>(b_screg.as<double>()), t, V, kern, width, part, d_corr);
        break;
      default:
        hipLaunchKernelGGL((k_reg_linearize<kRegGICP>), dim3(blocks), dim3(kRegThreads), 0, s, n_src, src[0], src[1], src[2],
                           static_cast<const double*>(b_screg.as<double>()), t, Q, kern, width, part, d_corr);
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

// what both entries refuse before a device is touched; *empty: the reference's early return applies
int reg_check(int method, const fdm_register_clouds* c, const double* T16, const fdm_align_settings& st, bool* empty) {
  *empty = false;
  if (!c) return fail(FDM_ERR_INVALID, "null argument");
  if (method < kRegICP || method > kRegGICP) return fail(FDM_ERR_INVALID, "method must be 0 (ICP), 1 (PLANE) or 2 (GICP)");
  if (st.robust_kernel < kRegNone || st.robust_kernel > kRegCauchy)
    return fail(FDM_ERR_INVALID, "robust_kernel must be 0 (NONE), 1 (HUBER), 2 (TUKEY) or 3 (CAUCHY)");
  if (!(st.max_correspondence_dist >= 0.0f)) return fail(FDM_ERR_INVALID, "max_correspondence_dist must not be negative or NaN");
  if (T16)
    for (int a = 0; a < 16; ++a)
      if (!std::isfinite(T16[a])) return fail(FDM_ERR_INVALID, "the transform has an entry that is not finite");
  if (int rc = check_cloud(c->n_source, c->sx, c->sy, c->sz)) return rc;
  if (int rc = check_cloud(c->n_target, c->tx, c->ty, c->tz)) return rc;
  if (c->n_source == 0 || c->n_target == 0) {
    *empty = true;
    return FDM_OK;
  }
  if (method == kRegPlane && (!c->tnx || !c->tny || !c->tnz))
    return fail(FDM_ERR_INVALID, "alignPlaneICP: target must have normals (all of nx, ny, nz)");
  if (method == kRegGICP && !c->s_cov9) return fail(FDM_ERR_INVALID, "alignGICP: source must have covariances");
  if (method == kRegGICP && !c->t_cov9) return fail(FDM_ERR_INVALID, "alignGICP: target must have covariances");
  return FDM_OK;
}
fdm_align_settings reg_settings(const fdm_align_settings* st) {
  fdm_align_settings d;
  fdm_default_align_settings(&d);
  return st ? *st : d;
}
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
  g_register_stats = fdm_register_stats{};
  if (!out) return fail(FDM_ERR_INVALID, "null argument");
  const fdm_align_settings st = reg_settings(settings);
  bool empty = false;
  if (int rc = reg_check(method, clouds, initial_guess, st, &empty)) return rc;
  const reg::Rigid guess = initial_guess ? reg::rigid_from_colmajor(initial_guess) : reg::rigid_identity();
  reg::Result R = reg::failed_result(guess, 0);  // the early return of an empty cloud (align.hpp:76-78)
  if (!empty) {
    const ScopedDevice restore;
    if (int rc = pick_device(device)) return rc;
    RegCall call;
    if (int rc = call.prepare(method, *clouds, st)) return rc;
    if (int rc = reg_solve(call, clouds->n_source, guess, st, &R)) return rc;
  }
  reg_write_result(R, out);
  return FDM_OK;
}

int fdm_cloud_register_linearize(int method, const fdm_register_clouds* clouds, const double* transform,
                                 const fdm_align_settings* settings, int device, double H[21], double b[6], double* error,
                                 uint64_t* num_inliers, int32_t* corr) {
  g_register_stats = fdm_register_stats{};
  if (!H || !b || !error || !num_inliers) return fail(FDM_ERR_INVALID, "null argument");
  const fdm_align_settings st = reg_settings(settings);
  bool empty = false;
  if (int rc = reg_check(method, clouds, transform, st, &empty)) return rc;
  reg::Model M;
  if (!empty) {
    const ScopedDevice restore;
    if (int rc = pick_device(device)) return rc;
    RegCall call;
    if (int rc = call.prepare(method, *clouds, st)) return rc;
    const bool host = clouds->on_device == 0;
    if (corr) {
      call.d_corr = corr;
      if (host) {
        if (int rc = call.b_corr.alloc(size_t(clouds->n_source) * sizeof(int32_t))) return rc;
        call.d_corr = call.b_corr.as<int32_t>();
      }
    }
    if (int rc = call.linearize(transform ? reg::rigid_from_colmajor(transform) : reg::rigid_identity(), M)) return rc;
    if (corr && host) HIPCK(hipMemcpy(corr, call.d_corr, size_t(clouds->n_source) * sizeof(int32_t), hipMemcpyDeviceToHost));
    call.finish();
  } else if (corr && clouds->n_source) {  // no target: nobody corresponds
    if (clouds->on_device) {
      const ScopedDevice restore;
      if (int rc = pick_device(device)) return rc;
      HIPCK(hipMemset(corr, 0xFF, size_t(clouds->n_source) * sizeof(int32_t)));
    } else {
      std::memset(corr, 0xFF, size_t(clouds->n_source) * sizeof(int32_t));
    }
  }
  std::memcpy(H, M.H, sizeof(M.H));
  std::memcpy(b, M.b, sizeof(M.b));
  *error = M.error;
  *num_inliers = M.num_inliers;
  return FDM_OK;
}

}  // extern "C"
