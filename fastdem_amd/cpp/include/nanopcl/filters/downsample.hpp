// nanopcl/filters/downsample.hpp — nanopcl::filters::voxelGrid and gridMaxZ of the reference
// (lib/nanoPCL/include/nanopcl/filters/downsample.hpp, impl/voxel_grid_impl.hpp, impl/grid_max_z_impl.hpp) over
// fdm_cloud_voxel_grid / fdm_cloud_grid_max_z: the SoA cloud's channels go to the device as they are, the filter runs
// there (include/fdm_engine.h states what every mode computes), the output keeps the input's channel layout, frame id and
// timestamp.  Both throw std::invalid_argument with the reference's texts for a size outside [0.001, 100].
//
// The order of the points inside a voxel — which decides NEAREST's and gridMaxZ's ties, ANY's pick and the rounding of
// the sums — follows a process-wide setting: 0 (default) = input order, 1 = the order libstdc++'s std::sort leaves, i.e.
// what a g++ build of the reference computes (FastDEM::setVoxelAnyOrder is the same switch for integrate()'s filter).
#pragma once
#include <atomic>
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>

#include "nanopcl/core.hpp"

namespace nanopcl {
namespace filters {

enum class VoxelMode { CENTROID, NEAREST, ANY, CENTER };

namespace detail {
inline std::atomic<int>& downsampleOrder() {
  static std::atomic<int> order{0};
  return order;
}

// mode < 0: gridMaxZ
inline PointCloud downsample(const PointCloud& cloud, float size, int mode) {
  PointCloud out;
  if (cloud.hasIntensity()) out.useIntensity();
  if (cloud.hasColor()) out.useColor();
  if (cloud.hasNormal()) out.useNormal();
  if (cloud.hasCovariance()) out.useCovariance();
  out.setFrameId(cloud.frameId());
  out.setTimestamp(cloud.timestamp());
  if (cloud.empty()) return out;
  out.resize(cloud.size());  // the call's capacity; cut to n_out below
  const fdm_cloud_view in{cloud.xData(), cloud.yData(), cloud.zData(), cloud.intensityData(), cloud.rgbData(),
                          cloud.normalData(0), cloud.normalData(1), cloud.normalData(2), cloud.covarianceData()};
  const fdm_cloud_out dst{out.xData(), out.yData(), out.zData(), out.intensityData(), out.rgbData(),
                          out.normalData(0), out.normalData(1), out.normalData(2), out.covarianceData(), nullptr};
  uint64_t n_out = 0;
  const int order = downsampleOrder().load(), device = 0;
  const int rc = mode < 0 ? fdm_cloud_grid_max_z(cloud.size(), &in, 0, size, order, device, &dst, &n_out)
                          : fdm_cloud_voxel_grid(cloud.size(), &in, 0, size, mode, order, device, &dst, &n_out);
  if (rc < 0) throw std::runtime_error(std::string(mode < 0 ? "gridMaxZ: " : "voxelGrid: ") + fdm_last_error());
  out.resize(size_t(n_out));
  return out;
}
inline bool sizeOk(float v) { return v >= 0.001f && v <= 100.0f; }  // voxel::MIN_SIZE, voxel::MAX_SIZE; NaN refused
}  // namespace detail

// 0 = ties in input order (default), 1 = the order std::sort leaves.  Process-wide.
inline void setDownsampleOrder(int order) { detail::downsampleOrder().store(order ? 1 : 0); }
inline int downsampleOrder() { return detail::downsampleOrder().load(); }

inline PointCloud voxelGrid(const PointCloud& cloud, float voxel_size, VoxelMode mode = VoxelMode::CENTROID) {
  if (!detail::sizeOk(voxel_size)) throw std::invalid_argument("voxel_size must be in [0.001, 100]");
  return detail::downsample(cloud, voxel_size, static_cast<int>(mode));
}
inline PointCloud voxelGrid(PointCloud&& cloud, float voxel_size, VoxelMode mode = VoxelMode::CENTROID) {
  if (!detail::sizeOk(voxel_size)) throw std::invalid_argument("voxel_size must be in [0.001, 100]");
  if (cloud.empty()) return std::move(cloud);  // voxel_grid_impl.hpp:34-35
  return detail::downsample(cloud, voxel_size, static_cast<int>(mode));
}

inline PointCloud gridMaxZ(const PointCloud& cloud, float grid_size) {
  if (!detail::sizeOk(grid_size)) throw std::invalid_argument("grid_size must be in [0.001, 100]");
  return detail::downsample(cloud, grid_size, -1);
}
inline PointCloud gridMaxZ(PointCloud&& cloud, float grid_size) {
  if (!detail::sizeOk(grid_size)) throw std::invalid_argument("grid_size must be in [0.001, 100]");
  return detail::downsample(cloud, grid_size, -1);
}

}  // namespace filters
}  // namespace nanopcl
