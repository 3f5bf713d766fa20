// fastdem/io/pcd_convert.hpp — a static point cloud into an ElevationMap and back
// (fastdem/include/fastdem/io/pcd_convert.hpp, src/pcd_convert.cpp:63-185, 327-373), on the device: the three calls
// forward to fdm_engine_from_point_cloud / fdm_engine_create_from_point_cloud / fdm_engine_to_point_cloud.
// No sensor model, transforms or estimator.  The offline DEM pipeline of the same reference header (DEMConfig, buildDEM:
// outlier removal, the per-cell histogram filter) is NOT declared here: it lives in fastdem/io/build_dem.hpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "fastdem/config/rasterization.hpp"
#include "fastdem/elevation_map.hpp"
#include "fastdem/point_types.hpp"

namespace fastdem {

/// Bins every point of a world-frame cloud into `map` (which has its geometry) and writes, per touched cell, elevation
/// (per `method`), elevation_min, elevation_max, variance (sample variance, Welford in input order), n_points, and
/// intensity (maximum) / color (last point) when the cloud has the channel; missing layers are created.  An empty
/// cloud, or one of which no point lands in the map, changes nothing.
inline void fromPointCloud(const PointCloud& cloud, ElevationMap& map, RasterMethod method = RasterMethod::Max) {
  if (cloud.empty()) return;
  if (!map.hasEngine()) throw nanogrid::EngineError("fromPointCloud: the map has no geometry");
  map.flushToDevice();
  const int rc = fdm_engine_from_point_cloud(map.engine(), cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(),
                                             cloud.intensityData(), cloud.rgbData(), static_cast<int>(method), nullptr);
  if (rc < 0) throw nanogrid::EngineError(std::string("fdm_engine_from_point_cloud: ") + fdm_last_error());
  if (rc == FDM_OK) map.invalidateHost();
}

/// The same into a new map that fits the cloud's x / y bounding box plus one cell.  An empty cloud gives a map without
/// geometry.  Throws when the box is not finite (no point with both coordinates, an infinite coordinate): the
/// reference's behaviour is undefined there.
inline ElevationMap fromPointCloud(const PointCloud& cloud, float resolution, RasterMethod method = RasterMethod::Max) {
  ElevationMap map;
  if (cloud.empty()) return map;
  fdm_engine* e = nullptr;
  const int rc = fdm_engine_create_from_point_cloud(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(),
                                                    cloud.intensityData(), cloud.rgbData(), 0, resolution,
                                                    static_cast<int>(method), 0, &e, nullptr);
  if (rc < 0) throw nanogrid::EngineError(std::string("fdm_engine_create_from_point_cloud: ") + fdm_last_error());
  if (e) map.adoptEngine(e);
  return map;
}

/// One point per cell whose elevation is not NaN: x, y the cell centre, z the elevation; intensity / colour channels
/// when some such cell has one (the others then carry 0 / black).
inline PointCloud toPointCloud(const ElevationMap& map) {
  PointCloud cloud;
  if (!map.hasEngine()) throw nanogrid::EngineError("toPointCloud: the map has no geometry");
  const_cast<ElevationMap&>(map).flushToDevice();
  const uint64_t cap = uint64_t(map.getSize()(0)) * uint64_t(map.getSize()(1));
  std::vector<float> x(cap), y(cap), z(cap), a(cap);
  std::vector<uint32_t> c(cap);
  uint64_t n = 0;
  int32_t has_intensity = 0, has_color = 0;
  const int rc = fdm_engine_to_point_cloud(map.engine(), cap, x.data(), y.data(), z.data(), a.data(), c.data(), &n,
                                           &has_intensity, &has_color);
  if (rc < 0) throw nanogrid::EngineError(std::string("fdm_engine_to_point_cloud: ") + fdm_last_error());
  cloud.reserve(n);
  for (uint64_t i = 0; i < n; ++i) cloud.add(x[i], y[i], z[i]);
  if (has_intensity) {
    cloud.useIntensity();
    for (uint64_t i = 0; i < n; ++i) cloud.intensity(i) = a[i];
  }
  if (has_color) {
    cloud.useColor();
    for (uint64_t i = 0; i < n; ++i)
      cloud.setColor(i, nanopcl::Color(uint8_t(c[i] >> 16), uint8_t(c[i] >> 8), uint8_t(c[i])));
  }
  return cloud;
}

}  // namespace fastdem
