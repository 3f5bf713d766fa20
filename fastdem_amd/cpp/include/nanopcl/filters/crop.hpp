// nanopcl/filters/crop.hpp — cropBox, cropRange, cropX / cropY / cropZ and cropAngle of the reference
// (lib/nanoPCL/include/nanopcl/filters/crop.hpp, impl/crop_impl.hpp) over fdm_cloud_crop: the predicate runs on the
// device, written as the reference writes it (include/fdm_engine.h states what a NaN does in each), the kept points are
// taken with PointCloud::extract.
#pragma once
#include "nanopcl/filters/core.hpp"

namespace nanopcl {
namespace filters {

[[nodiscard]] inline PointCloud cropBox(const PointCloud& cloud, const Point& min, const Point& max,
                                        FilterMode mode = FilterMode::INSIDE) {
  const float lo[3] = {min.x(), min.y(), min.z()}, hi[3] = {max.x(), max.y(), max.z()};
  return detail::crop(cloud, FDM_CROP_BOX, mode, lo, hi, "cropBox");
}
[[nodiscard]] inline PointCloud cropBox(PointCloud&& cloud, const Point& min, const Point& max,
                                        FilterMode mode = FilterMode::INSIDE) {
  const PointCloud& in = cloud;
  return cropBox(in, min, max, mode);
}

[[nodiscard]] inline PointCloud cropRange(const PointCloud& cloud, float min_range, float max_range,
                                          FilterMode mode = FilterMode::INSIDE) {
  return detail::crop(cloud, FDM_CROP_RANGE, mode, min_range, max_range, "cropRange");
}
[[nodiscard]] inline PointCloud cropRange(PointCloud&& cloud, float min_range, float max_range,
                                          FilterMode mode = FilterMode::INSIDE) {
  const PointCloud& in = cloud;
  return cropRange(in, min_range, max_range, mode);
}

[[nodiscard]] inline PointCloud cropX(const PointCloud& cloud, float min, float max, FilterMode mode = FilterMode::INSIDE) {
  return detail::crop(cloud, FDM_CROP_X, mode, min, max, "cropX");
}
[[nodiscard]] inline PointCloud cropX(PointCloud&& cloud, float min, float max, FilterMode mode = FilterMode::INSIDE) {
  const PointCloud& in = cloud;
  return cropX(in, min, max, mode);
}

[[nodiscard]] inline PointCloud cropY(const PointCloud& cloud, float min, float max, FilterMode mode = FilterMode::INSIDE) {
  return detail::crop(cloud, FDM_CROP_Y, mode, min, max, "cropY");
}
[[nodiscard]] inline PointCloud cropY(PointCloud&& cloud, float min, float max, FilterMode mode = FilterMode::INSIDE) {
  const PointCloud& in = cloud;
  return cropY(in, min, max, mode);
}

[[nodiscard]] inline PointCloud cropZ(const PointCloud& cloud, float min, float max, FilterMode mode = FilterMode::INSIDE) {
  return detail::crop(cloud, FDM_CROP_Z, mode, min, max, "cropZ");
}
[[nodiscard]] inline PointCloud cropZ(PointCloud&& cloud, float min, float max, FilterMode mode = FilterMode::INSIDE) {
  const PointCloud& in = cloud;
  return cropZ(in, min, max, mode);
}

/// The azimuth sector from min_angle to max_angle (radians); min_angle > max_angle wraps through pi.
[[nodiscard]] inline PointCloud cropAngle(const PointCloud& cloud, float min_angle, float max_angle,
                                          FilterMode mode = FilterMode::INSIDE) {
  return detail::crop(cloud, FDM_CROP_ANGLE, mode, min_angle, max_angle, "cropAngle");
}
[[nodiscard]] inline PointCloud cropAngle(PointCloud&& cloud, float min_angle, float max_angle,
                                          FilterMode mode = FilterMode::INSIDE) {
  const PointCloud& in = cloud;
  return cropAngle(in, min_angle, max_angle, mode);
}

}  // namespace filters
}  // namespace nanopcl
