// nanopcl/filters/outlier_removal.hpp — radiusOutlierRemoval of the reference
// (lib/nanoPCL/include/nanopcl/filters/outlier_removal.hpp, impl/outlier_removal_impl.hpp:21-77) over
// fdm_cloud_radius_outlier_removal: the keep mask comes from the device (mask mode: a point's search stops at
// min_neighbors), the kept points are taken with PointCloud::extract.  statisticalOutlierRemoval lives in
// fastdem/io/build_dem.hpp, beside buildDEM, which starts with it; this header brings it along.
#pragma once
#include "fastdem/io/build_dem.hpp"
#include "nanopcl/filters/core.hpp"

namespace nanopcl {
namespace filters {

/// The points with at least min_neighbors OTHER points within `radius` (by index: a duplicate counts), in input order, with
/// every channel the cloud carries, its frame id and its timestamp.  An empty cloud gives an empty cloud.  A radius that is
/// not a positive finite number, a coordinate that is not finite (removeInvalid first), a cloud farther than 2^20 radii
/// from the origin or one too dense for the radius (include/fdm_engine.h) throw std::runtime_error.
[[nodiscard]] inline PointCloud radiusOutlierRemoval(const PointCloud& cloud, float radius, size_t min_neighbors) {
  if (cloud.empty()) return PointCloud();
  std::vector<uint8_t> keep(cloud.size(), 0);
  uint64_t n_kept = 0;
  const int rc = fdm_cloud_radius_outlier_removal(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, radius,
                                                  min_neighbors, 0, keep.data(), nullptr, &n_kept);
  if (rc < 0) throw std::runtime_error(std::string("radiusOutlierRemoval: ") + fdm_last_error());
  return detail::extractKept(cloud, keep, n_kept);
}
[[nodiscard]] inline PointCloud radiusOutlierRemoval(PointCloud&& cloud, float radius, size_t min_neighbors) {
  if (cloud.empty()) return std::move(cloud);
  const PointCloud& in = cloud;
  return radiusOutlierRemoval(in, radius, min_neighbors);
}

}  // namespace filters
}  // namespace nanopcl
