// nanopcl/registration/vgicp.hpp — nanopcl::registration::VoxelDistribution, VoxelDistributionMap, VoxelCorrespondence and
// both alignVGICP overloads of the reference (lib/nanoPCL/include/nanopcl/registration/voxel_distribution_map.hpp,
// correspondence/voxel_correspondence.hpp:30-82, align.hpp:276-353) over fdm_voxel_map_create and
// fdm_cloud_register_vgicp: the map is built and kept on the device, a registration is one lookup per source point and
// iteration there (include/fdm_engine.h states what is computed, the voxel order, the regularised covariance and its
// deviation from the reference's float eigen-solver included).  Signatures, defaults, early returns and the exception
// text for a source without covariances are the reference's.
//
// OPT-IN.  nanopcl/registration.hpp on its own still declares both alignVGICP overloads deleted.  This header defines
// NANOPCL_VGICP and includes it, so it has to come FIRST — before nanopcl/core.hpp, which pulls registration.hpp in — or
// the translation unit is compiled with -DNANOPCL_VGICP.
//
// A map object owns an fdm_voxel_map and is move-only.  build() also downloads the records once; lookup() and
// lookupRegularized() answer on the host, by the same pack and a binary search over the ascending keys
// (vgicp_lookup.hpp); lookupRegularized returns C_reg rounded to float.  Not mirrored: VoxelCorrespondence::find and
// DistributionContext — the mirror carries no factor types.
#pragma once
#if defined(NANOPCL_REGISTRATION_VGICP_DELETED)
#error "nanopcl/registration.hpp was included before nanopcl/registration/vgicp.hpp and has declared alignVGICP deleted: include nanopcl/registration/vgicp.hpp first, or compile with -DNANOPCL_VGICP"
#endif
#ifndef NANOPCL_VGICP
#define NANOPCL_VGICP
#endif
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "nanopcl/registration.hpp"
#include "nanopcl/registration/vgicp_lookup.hpp"

namespace nanopcl {
namespace registration {

struct VoxelDistribution {
  Eigen::Vector3f mean;        // centroid of the voxel's points
  Eigen::Matrix3f covariance;  // of its points; float(eps) * I for fewer than three
  uint32_t num_points;
  [[nodiscard]] bool isValid() const { return num_points >= 1; }
  [[nodiscard]] bool hasFullCovariance() const { return num_points >= 3; }
};

class VoxelDistributionMap {
 public:
  explicit VoxelDistributionMap(float resolution = 0.5f, double covariance_epsilon = 1e-3)
      : resolution_(resolution), inv_resolution_(1.0f / resolution), covariance_epsilon_(covariance_epsilon) {}
  ~VoxelDistributionMap() { fdm_voxel_map_destroy(map_); }
  VoxelDistributionMap(const VoxelDistributionMap&) = delete;
  VoxelDistributionMap& operator=(const VoxelDistributionMap&) = delete;
  VoxelDistributionMap(VoxelDistributionMap&& o) noexcept { *this = std::move(o); }
  VoxelDistributionMap& operator=(VoxelDistributionMap&& o) noexcept {
    if (this != &o) {
      fdm_voxel_map_destroy(map_);
      map_ = std::exchange(o.map_, nullptr);
      resolution_ = o.resolution_;
      inv_resolution_ = o.inv_resolution_;
      covariance_epsilon_ = o.covariance_epsilon_;
      keys_ = std::move(o.keys_); mean_ = std::move(o.mean_); cov_ = std::move(o.cov_);
      creg_ = std::move(o.creg_); count_ = std::move(o.count_);
      o.clear();
    }
    return *this;
  }

  // the map of `cloud` on `device`, and its records on the host; an empty cloud gives an empty map
  void build(const PointCloud& cloud, int device = 0) {
    fdm_voxel_map_destroy(map_);
    map_ = nullptr;
    clear();
    if (cloud.empty()) return;
    if (fdm_voxel_map_create(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, resolution_,
                             covariance_epsilon_, device, &map_) < 0)
      throw std::runtime_error(std::string("VoxelDistributionMap::build: ") + fdm_last_error());
    fdm_voxel_map_info info;
    if (fdm_voxel_map_get_info(map_, &info) < 0)
      throw std::runtime_error(std::string("VoxelDistributionMap::build: ") + fdm_last_error());
    const size_t n = size_t(info.num_voxels);
    keys_.resize(n); mean_.resize(3 * n); cov_.resize(9 * n); creg_.resize(6 * n); count_.resize(n);
    if (fdm_voxel_map_records(map_, 0, keys_.data(), mean_.data(), cov_.data(), creg_.data(), count_.data()) < 0)
      throw std::runtime_error(std::string("VoxelDistributionMap::build: ") + fdm_last_error());
  }

  [[nodiscard]] std::optional<VoxelDistribution> lookup(const Point& p) const {
    const size_t at = find(p);
    if (at == keys_.size()) return std::nullopt;
    VoxelDistribution d = head(at);
    for (int c = 0; c < 3; ++c)
      for (int r = 0; r < 3; ++r) d.covariance(r, c) = cov_[9 * at + size_t(c * 3 + r)];
    return d;
  }
  // ... with the pre-regularised covariance, eigenvalues (eps, 1, 1): C_reg rounded to float
  [[nodiscard]] std::optional<VoxelDistribution> lookupRegularized(const Point& p) const {
    const size_t at = find(p);
    if (at == keys_.size()) return std::nullopt;
    VoxelDistribution d = head(at);
    const double* g = &creg_[6 * at];  // xx, xy, xz, yy, yz, zz
    const double full[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], g[5]}};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) d.covariance(r, c) = float(full[r][c]);
    return d;
  }

  [[nodiscard]] float resolution() const noexcept { return resolution_; }
  [[nodiscard]] float invResolution() const noexcept { return inv_resolution_; }
  [[nodiscard]] size_t numVoxels() const noexcept { return keys_.size(); }
  [[nodiscard]] bool empty() const noexcept { return keys_.empty(); }
  [[nodiscard]] double covarianceEpsilon() const noexcept { return covariance_epsilon_; }
  [[nodiscard]] const fdm_voxel_map* handle() const noexcept { return map_; }  // null for an empty map

 private:
  void clear() { keys_.clear(); mean_.clear(); cov_.clear(); creg_.clear(); count_.clear(); }
  size_t find(const Point& p) const {
    return detail::vgicp_find(keys_.data(), keys_.size(), detail::vgicp_pack(p(0), p(1), p(2), inv_resolution_));
  }
  VoxelDistribution head(size_t at) const {
    VoxelDistribution d;
    for (int a = 0; a < 3; ++a) d.mean(a) = mean_[3 * at + size_t(a)];
    d.num_points = count_[at];
    return d;
  }

  float resolution_, inv_resolution_;
  double covariance_epsilon_;
  fdm_voxel_map* map_ = nullptr;
  std::vector<uint64_t> keys_;   // ascending
  std::vector<float> mean_, cov_;
  std::vector<double> creg_;
  std::vector<uint32_t> count_;
};

class VoxelCorrespondence {
 public:
  explicit VoxelCorrespondence(float resolution = 1.0f, double epsilon = 1e-3) : voxel_map_(resolution, epsilon) {}
  void build(const PointCloud& target, int device = 0) { voxel_map_.build(target, device); }
  [[nodiscard]] bool empty() const { return voxel_map_.empty(); }
  [[nodiscard]] const VoxelDistributionMap& voxelMap() const { return voxel_map_; }

 private:
  VoxelDistributionMap voxel_map_;
};

// alignVGICP against a prebuilt map (align.hpp:276-323): the fast path of scan-to-map registration
[[nodiscard]] inline RegistrationResult alignVGICP(const PointCloud& source, const VoxelCorrespondence& correspondence,
                                                   const Eigen::Isometry3d& initial_guess = Eigen::Isometry3d::Identity(),
                                                   const AlignSettings& settings = {}) {
  if (source.empty() || correspondence.empty()) return detail::empty_result(initial_guess);
  if (!source.hasCovariance())
    throw std::runtime_error("alignVGICP: source must have covariances. Call geometry::estimateCovariances() first.");
  const fdm_align_settings st = detail::to_settings(settings);
  fdm_registration_result r;
  const int rc = fdm_cloud_register_vgicp(correspondence.voxelMap().handle(), source.size(), source.xData(), source.yData(),
                                          source.zData(), source.covarianceData(), 0, initial_guess.matrix().data(), &st, &r);
  if (rc < 0) throw std::runtime_error(std::string("alignVGICP: ") + fdm_last_error());
  return detail::to_result(r);
}

// ... building the map for this call alone (align.hpp:337-353)
[[nodiscard]] inline RegistrationResult alignVGICP(const PointCloud& source, const PointCloud& target,
                                                   float voxel_resolution = 1.0f,
                                                   const Eigen::Isometry3d& initial_guess = Eigen::Isometry3d::Identity(),
                                                   const AlignSettings& settings = {}) {
  if (source.empty() || target.empty()) return detail::empty_result(initial_guess);
  VoxelCorrespondence correspondence(voxel_resolution, settings.covariance_epsilon);
  correspondence.build(target);
  return alignVGICP(source, correspondence, initial_guess, settings);
}

}  // namespace registration
}  // namespace nanopcl
