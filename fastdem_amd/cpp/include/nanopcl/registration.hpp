// nanopcl/registration.hpp — nanopcl::registration::alignICP, alignPlaneICP and alignGICP of the reference
// (lib/nanoPCL/include/nanopcl/registration/align.hpp:71-246) with its AlignSettings (:32-59), RobustKernel
// (factors/robust_kernels.hpp:24-29) and RegistrationResult (result.hpp:27-60), over fdm_cloud_register: the clouds'
// channels go to the device as they are, the per-iteration work runs there, the 6 x 6 algebra on the host
// (include/fdm_engine.h states what is computed, the covariance rule and the eps names included).  Signatures, defaults and
// the exceptions for a missing normal or covariance channel are the reference's; an empty cloud returns before the
// channels are looked at, as there.
//
// Not mirrored: IterativeSolver, the factors, linearizers and correspondence classes as types of their own (one
// linearization is fdm_cloud_register_linearize).  alignVGICP and the voxel distribution map are OPT-IN: they live in
// nanopcl/registration/vgicp.hpp, which defines NANOPCL_VGICP and includes this header.  Without that macro both
// overloads are declared deleted here, so that a call fails at compile time with their name.
#pragma once
#include <cstddef>
#include <cstring>
#include <limits>
#include <optional>
#include <stdexcept>
#include <string>

#include "nanopcl/core.hpp"

namespace nanopcl {
namespace registration {

using Matrix6d = Eigen::Matrix<double, 6, 6>;
using Vector6d = Eigen::Matrix<double, 6, 1>;

enum class RobustKernel { NONE, HUBER, TUKEY, CAUCHY };

struct AlignSettings {
  float max_correspondence_dist = 1.0f;
  int max_iterations = 50;
  double translation_eps = 1e-4;  // (criteria.hpp compares it with the twist's LAST three: see include/fdm_engine.h)
  double rotation_eps = 1e-4;
  double relative_error_eps = 1e-6;
  size_t min_correspondences = 10;
  RobustKernel robust_kernel = RobustKernel::NONE;
  double robust_kernel_width = 1.0;
  double covariance_epsilon = 1e-3;
};

struct RegistrationResult {
  Eigen::Isometry3d transform;
  double fitness;
  double rmse;
  size_t iterations;
  bool converged;
  std::optional<Matrix6d> covariance;  // [v; omega] order; absent where H is not safely positive definite

  bool success(double min_fitness = 0.5) const noexcept { return converged && fitness >= min_fitness; }
  std::optional<Matrix6d> informationMatrix() const {
    if (!covariance) return std::nullopt;
    return covariance->inverse();
  }
};

namespace detail {
inline fdm_align_settings to_settings(const AlignSettings& settings) {
  fdm_align_settings st;
  fdm_default_align_settings(&st);
  st.max_correspondence_dist = settings.max_correspondence_dist;  // (carried by every method; VGICP does not use it)
  st.max_iterations = settings.max_iterations;
  st.translation_eps = settings.translation_eps;
  st.rotation_eps = settings.rotation_eps;
  st.relative_error_eps = settings.relative_error_eps;
  st.min_correspondences = settings.min_correspondences;
  st.robust_kernel = int(settings.robust_kernel);
  st.robust_kernel_width = settings.robust_kernel_width;
  st.covariance_epsilon = settings.covariance_epsilon;
  return st;
}
inline RegistrationResult to_result(const fdm_registration_result& r) {
  RegistrationResult out{Eigen::Isometry3d::Identity(), r.fitness, r.rmse, size_t(r.iterations), r.converged != 0, std::nullopt};
  std::memcpy(out.transform.data(), r.transform, sizeof(r.transform));  // both column-major 4 x 4
  if (r.has_covariance) {
    Matrix6d cov;
    for (int row = 0; row < 6; ++row)
      for (int col = 0; col < 6; ++col) cov(row, col) = r.covariance[row * 6 + col];
    out.covariance = cov;
  }
  return out;
}
inline RegistrationResult align(int method, const PointCloud& source, const PointCloud& target,
                                const Eigen::Isometry3d& initial_guess, const AlignSettings& settings, const char* who) {
  const fdm_align_settings st = to_settings(settings);
  fdm_register_clouds c{};
  c.n_source = source.size();
  c.sx = source.xData(); c.sy = source.yData(); c.sz = source.zData();
  c.s_cov9 = method == FDM_REGISTER_GICP ? source.covarianceData() : nullptr;
  c.n_target = target.size();
  c.tx = target.xData(); c.ty = target.yData(); c.tz = target.zData();
  if (method == FDM_REGISTER_PLANE) { c.tnx = target.normalData(0); c.tny = target.normalData(1); c.tnz = target.normalData(2); }
  c.t_cov9 = method == FDM_REGISTER_GICP ? target.covarianceData() : nullptr;
  c.on_device = 0;
  const int device = 0;
  fdm_registration_result r;
  const int rc = fdm_cloud_register(method, &c, initial_guess.matrix().data(), &st, device, &r);
  if (rc < 0) throw std::runtime_error(std::string(who) + ": " + fdm_last_error());
  return to_result(r);
}
inline RegistrationResult empty_result(const Eigen::Isometry3d& initial_guess) {  // align.hpp:76-78
  return {initial_guess, 0.0, std::numeric_limits<double>::infinity(), 0, false, std::nullopt};
}
}  // namespace detail

[[nodiscard]] inline RegistrationResult alignICP(const PointCloud& source, const PointCloud& target,
                                                 const Eigen::Isometry3d& initial_guess = Eigen::Isometry3d::Identity(),
                                                 const AlignSettings& settings = {}) {
  if (source.empty() || target.empty()) return detail::empty_result(initial_guess);
  return detail::align(FDM_REGISTER_ICP, source, target, initial_guess, settings, "alignICP");
}

[[nodiscard]] inline RegistrationResult alignPlaneICP(const PointCloud& source, const PointCloud& target,
                                                      const Eigen::Isometry3d& initial_guess = Eigen::Isometry3d::Identity(),
                                                      const AlignSettings& settings = {}) {
  if (source.empty() || target.empty()) return detail::empty_result(initial_guess);
  if (!target.hasNormal())
    throw std::runtime_error("alignPlaneICP: target must have normals. Call geometry::estimateNormals() first.");
  return detail::align(FDM_REGISTER_PLANE, source, target, initial_guess, settings, "alignPlaneICP");
}

[[nodiscard]] inline RegistrationResult alignGICP(const PointCloud& source, const PointCloud& target,
                                                  const Eigen::Isometry3d& initial_guess = Eigen::Isometry3d::Identity(),
                                                  const AlignSettings& settings = {}) {
  if (source.empty() || target.empty()) return detail::empty_result(initial_guess);
  if (!source.hasCovariance())
    throw std::runtime_error("alignGICP: source must have covariances. Call geometry::estimateCovariances() first.");
  if (!target.hasCovariance())
    throw std::runtime_error("alignGICP: target must have covariances. Call geometry::estimateCovariances() first.");
  return detail::align(FDM_REGISTER_GICP, source, target, initial_guess, settings, "alignGICP");
}

#ifndef NANOPCL_VGICP
#define NANOPCL_REGISTRATION_VGICP_DELETED
// the reference's voxelized GICP (align.hpp:276-353): provided by nanopcl/registration/vgicp.hpp, not by this header alone
class VoxelCorrespondence;
RegistrationResult alignVGICP(const PointCloud& source, const VoxelCorrespondence& correspondence,
                              const Eigen::Isometry3d& initial_guess = Eigen::Isometry3d::Identity(),
                              const AlignSettings& settings = {}) = delete;
RegistrationResult alignVGICP(const PointCloud& source, const PointCloud& target, float voxel_resolution = 1.0f,
                              const Eigen::Isometry3d& initial_guess = Eigen::Isometry3d::Identity(),
                              const AlignSettings& settings = {}) = delete;
#endif

}  // namespace registration
}  // namespace nanopcl
