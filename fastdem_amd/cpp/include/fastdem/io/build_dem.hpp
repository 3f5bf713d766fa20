// fastdem/io/build_dem.hpp — the offline DEM pipeline of the reference's fastdem/io/pcd_convert.hpp (DEMConfig, buildDEM:
// src/pcd_convert.cpp:194-323) and the nanoPCL filter it starts with (nanopcl::filters::statisticalOutlierRemoval,
// outlier_removal_impl.hpp:83-142), on the device: they forward to fdm_engine_build_dem and
// fdm_statistical_outlier_removal.  A header of its own: a caller of the reference that uses buildDEM includes this one
// beside fastdem/io/pcd_convert.hpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "fastdem/io/pcd_convert.hpp"

namespace nanopcl {
namespace filters {

/// The points whose mean distance to their k nearest neighbours is at most (global mean + std_mul * global deviation),
/// in input order, with every channel the cloud carries, its frame id and its timestamp.  k == 0, an empty cloud or a
/// single point give an empty cloud.  The neighbour search is exact; more than 64 effective neighbours, or a coordinate
/// that is not finite, throw.
inline PointCloud statisticalOutlierRemoval(const PointCloud& cloud, size_t k, float std_mul = 1.0f) {
  if (cloud.empty() || k == 0) return PointCloud();
  const size_t n = cloud.size();
  std::vector<uint8_t> keep(n, 0);
  float threshold = 0.0f;
  uint64_t n_kept = 0;
  const int rc = fdm_statistical_outlier_removal(n, cloud.xData(), cloud.yData(), cloud.zData(), 0,
                                                 k > size_t(1) << 30 ? -1 : int(k), std_mul, 0, keep.data(), nullptr,
                                                 &threshold, &n_kept);
  if (rc < 0) throw nanogrid::EngineError(std::string("fdm_statistical_outlier_removal: ") + fdm_last_error());
  PointCloud out;
  out.reserve(n_kept);
  for (size_t i = 0; i < n; ++i)
    if (keep[i]) out.add(cloud.xData()[i], cloud.yData()[i], cloud.zData()[i]);
  if (cloud.hasIntensity()) {
    out.useIntensity();
    for (size_t i = 0, o = 0; i < n; ++i)
      if (keep[i]) out.intensity(o++) = cloud.intensity(i);
  }
  if (cloud.hasColor()) {
    out.useColor();
    for (size_t i = 0, o = 0; i < n; ++i)
      if (keep[i]) out.setColor(o++, cloud.color(i));
  }
  if (cloud.hasCovariance()) {
    out.useCovariance();
    float* const dst = out.covarianceData();
    for (size_t i = 0, o = 0; i < n; ++i) {
      if (!keep[i]) continue;
      const Eigen::Matrix3f m = cloud.covariance(i);
      for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) dst[o * 9 + size_t(c) * 3 + size_t(r)] = m(r, c);
      ++o;
    }
  }
  if (n_kept) {  // (the reference's early returns hand back a default-constructed cloud)
    out.setFrameId(cloud.frameId());
    out.setTimestamp(cloud.timestamp());
  }
  return out;
}

}  // namespace filters
}  // namespace nanopcl

namespace fastdem {

/// Configuration for buildDEM(): the reference's fields and defaults.
struct DEMConfig {
  float resolution = 0.1f;
  RasterMethod method = RasterMethod::Max;
  int sor_k = 10;                 ///< neighbours of the statistical outlier removal (at most 64 effective)
  float sor_std_mul = 1.0f;       ///< standard deviation multiplier of its threshold
  float height_threshold = 2.0f;  ///< metres above a cell's ground peak from which points are removed
  float bin_size = 0.0f;          ///< histogram bin; 0 = the resolution
  int inpaint_iterations = 3;     ///< inpainting passes (0 = none)
};

/// Outlier removal, per-cell floating-point removal, rasterization and inpainting of a merged world-frame cloud, all on
/// the device.  An empty cloud, or one the outlier removal empties, gives a map without geometry.
inline ElevationMap buildDEM(const PointCloud& cloud, const DEMConfig& config = {}) {
  ElevationMap map;
  if (cloud.empty()) return map;
  fdm_dem_config c;
  c.resolution = config.resolution;
  c.method = static_cast<int32_t>(config.method);
  c.sor_k = config.sor_k;
  c.sor_std_mul = config.sor_std_mul;
  c.height_threshold = config.height_threshold;
  c.bin_size = config.bin_size;
  c.inpaint_iterations = config.inpaint_iterations;
  fdm_engine* e = nullptr;
  const int rc = fdm_engine_build_dem(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), cloud.intensityData(),
                                      cloud.rgbData(), 0, &c, 0, &e, nullptr);
  if (rc < 0) throw nanogrid::EngineError(std::string("fdm_engine_build_dem: ") + fdm_last_error());
  if (e) map.adoptEngine(e);
  return map;
}

}  // namespace fastdem
