// nanopcl/filters/core.hpp — FilterMode, the generic filter(cloud, pred) and removeInvalid of the reference
// (lib/nanoPCL/include/nanopcl/filters/core.hpp).  filter() runs its predicate on the host, as the reference does: a
// predicate is the caller's code.  removeInvalid, the crops (crop.hpp) and radiusOutlierRemoval (outlier_removal.hpp)
// get a keep mask from the device (fdm_cloud_crop / fdm_cloud_radius_outlier_removal, include/fdm_engine.h) and take the
// kept points with PointCloud::extract: every channel the cloud carries, its frame id and its timestamp stay.  The &&
// overloads return the same cloud as the const& ones.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "nanopcl/core.hpp"

namespace nanopcl {
namespace filters {

enum class FilterMode { INSIDE, OUTSIDE };

namespace detail {
// the points a mask keeps, in input order
inline PointCloud extractKept(const PointCloud& cloud, const std::vector<uint8_t>& keep, uint64_t n_kept) {
  std::vector<size_t> idx;
  idx.reserve(size_t(n_kept));
  for (size_t i = 0; i < keep.size(); ++i)
    if (keep[i]) idx.push_back(i);
  return cloud.extract(idx);
}

// fdm_cloud_crop over a host cloud
inline PointCloud crop(const PointCloud& cloud, int kind, FilterMode mode, const float lo[3], const float hi[3],
                       const char* who) {
  fdm_crop_config cfg{};
  cfg.kind = kind;
  cfg.mode = mode == FilterMode::INSIDE ? FDM_CROP_INSIDE : FDM_CROP_OUTSIDE;
  for (int k = 0; k < 3; ++k) { cfg.lo[k] = lo[k]; cfg.hi[k] = hi[k]; }
  std::vector<uint8_t> keep(cloud.size(), 0);
  uint64_t n_kept = 0;
  const int rc = fdm_cloud_crop(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, &cfg, 0, keep.data(), &n_kept);
  if (rc < 0) throw std::runtime_error(std::string(who) + ": " + fdm_last_error());
  return extractKept(cloud, keep, n_kept);
}
inline PointCloud crop(const PointCloud& cloud, int kind, FilterMode mode, float lo, float hi, const char* who) {
  const float l[3] = {lo, 0.0f, 0.0f}, h[3] = {hi, 0.0f, 0.0f};
  return crop(cloud, kind, mode, l, h, who);
}
}  // namespace detail

/// Generic filter: Predicate = bool(size_t index), evaluated on the host.
template <typename Predicate>
[[nodiscard]] inline PointCloud filter(const PointCloud& cloud, Predicate pred) {
  std::vector<size_t> idx;
  idx.reserve(cloud.size());
  for (size_t i = 0; i < cloud.size(); ++i)
    if (pred(i)) idx.push_back(i);
  return cloud.extract(idx);
}
template <typename Predicate>
[[nodiscard]] inline PointCloud filter(PointCloud&& cloud, Predicate pred) {
  const PointCloud& in = cloud;
  return filter(in, pred);
}

/// The points whose three coordinates are finite.
[[nodiscard]] inline PointCloud removeInvalid(const PointCloud& cloud) {
  return detail::crop(cloud, FDM_CROP_FINITE, FilterMode::INSIDE, 0.0f, 0.0f, "removeInvalid");
}
[[nodiscard]] inline PointCloud removeInvalid(PointCloud&& cloud) {
  const PointCloud& in = cloud;
  return removeInvalid(in);
}

}  // namespace filters
}  // namespace nanopcl
