// nanopcl/geometry/normal_estimation.hpp — nanopcl::geometry::estimateNormals, estimateCovariances and
// estimateNormalsCovariances of the reference (lib/nanoPCL/include/nanopcl/geometry/normal_estimation.hpp:43-63, 107-124,
// 159-179) in their k-NN form, over fdm_cloud_estimate_normals: the cloud's x / y / z channels go to the device as they
// are, the search and the PCA run there (include/fdm_engine.h states what is computed), and the normal / covariance
// channels are filled in place.  The channels are enabled as the reference's setters' prepare() does; an empty cloud
// returns before anything is enabled.
//
// Not mirrored: the overloads that take a pre-built search::KdTree (the mirror has none: call the plain overload), and
// the radius overloads.  The latter are declared deleted on purpose — with only the int overloads visible,
// estimateNormals(cloud, 0.5f) would silently convert the radius to k = 0.
#pragma once
#include <stdexcept>
#include <string>

#include "nanopcl/core.hpp"

namespace nanopcl {
namespace geometry {

namespace detail {
inline void estimate(PointCloud& cloud, int k, const Point* viewpoint, bool normals, bool covariances, const char* who) {
  if (cloud.empty()) return;
  if (normals) cloud.useNormal();
  if (covariances) cloud.useCovariance();
  const float vp[3] = {viewpoint ? viewpoint->x() : 0.0f, viewpoint ? viewpoint->y() : 0.0f,
                       viewpoint ? viewpoint->z() : 0.0f};
  const int device = 0;
  const int rc = fdm_cloud_estimate_normals(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, k, vp, device,
                                            normals ? cloud.normalData(0) : nullptr, normals ? cloud.normalData(1) : nullptr,
                                            normals ? cloud.normalData(2) : nullptr,
                                            covariances ? cloud.covarianceData() : nullptr, nullptr);
  if (rc < 0) throw std::runtime_error(std::string(who) + ": " + fdm_last_error());
}
}  // namespace detail

inline void estimateNormals(PointCloud& cloud, int k = 20, const Point& viewpoint = Point::Zero()) {
  detail::estimate(cloud, k, &viewpoint, true, false, "estimateNormals");
}
inline void estimateCovariances(PointCloud& cloud, int k = 20) {
  detail::estimate(cloud, k, nullptr, false, true, "estimateCovariances");
}
inline void estimateNormalsCovariances(PointCloud& cloud, int k = 20, const Point& viewpoint = Point::Zero()) {
  detail::estimate(cloud, k, &viewpoint, true, true, "estimateNormalsCovariances");
}

// the reference's radius overloads (VoxelHash search): not provided
size_t estimateNormals(PointCloud& cloud, float radius, const Point& viewpoint = Point::Zero()) = delete;
size_t estimateCovariances(PointCloud& cloud, float radius) = delete;
size_t estimateNormalsCovariances(PointCloud& cloud, float radius, const Point& viewpoint = Point::Zero()) = delete;

}  // namespace geometry
}  // namespace nanopcl
