// nanopcl/segmentation.hpp — nanopcl::segmentation::segmentGround, segmentPlane and segmentMultiplePlanes of the reference
// (lib/nanoPCL/include/nanopcl/segmentation/ground_seg.hpp:34-106, ransac_plane.hpp:41-158) over
// fdm_cloud_segment_ground / _plane / _planes: the cloud's x, y, z channels go to the device as they are, the cells'
// sorts and the hypotheses' scoring run there (include/fdm_engine.h states what is computed, the refinement's summation
// order and the refined normal's sign included).  Names, signatures and defaults are the reference's.  PlaneModel's own
// arithmetic (fromPoints, signedDistance, distance, isValid) runs on the host, in the order the header states.
//
// Not mirrored: euclideanCluster and applyClusterLabels — the clusters' order follows the iteration order of a voxel hash
// and an unstable std::sort, which cannot be restated; the function is declared deleted so that a call fails at compile
// time with its name.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "nanopcl/core.hpp"

namespace nanopcl {
namespace segmentation {

struct PlaneModel {  // ransac_plane.hpp:41-68
  Point4 coefficients{0.f, 0.f, 1.f, 0.f};  // [nx, ny, nz, d]: n . p + d = 0

  [[nodiscard]] float signedDistance(const Point& p) const noexcept {
    const float nx = coefficients[0], ny = coefficients[1], nz = coefficients[2];
    return ((nx * p[0] + ny * p[1]) + nz * p[2]) + coefficients[3];
  }
  [[nodiscard]] float distance(const Point& p) const noexcept { return std::abs(signedDistance(p)); }
  [[nodiscard]] bool isValid() const noexcept { return std::isfinite(coefficients[3]); }

  // ransac_plane_impl.hpp:196-215; three-term sums as a0 + (a1 + a2) (include/fdm_engine.h)
  [[nodiscard]] static PlaneModel fromPoints(const Point& p1, const Point& p2, const Point& p3) {
    const float a[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const float b[3] = {p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2]};
    float n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const float norm = std::sqrt(n[0] * n[0] + (n[1] * n[1] + n[2] * n[2]));
    PlaneModel m;
    if (norm < 1e-10f) {  // collinear points: an invalid plane
      m.coefficients = Point4(0.f, 0.f, 0.f, std::numeric_limits<float>::quiet_NaN());
      return m;
    }
    for (float& c : n) c /= norm;
    m.coefficients = Point4(n[0], n[1], n[2], -(n[0] * p1[0] + (n[1] * p1[1] + n[2] * p1[2])));
    return m;
  }
};

struct RansacResult {  // ransac_plane.hpp:77-95
  PlaneModel model;
  std::vector<uint32_t> inliers;
  double fitness{0.0};
  int iterations{0};

  [[nodiscard]] std::vector<uint32_t> outliers(size_t total_points) const {  // ransac_plane_impl.hpp:221-235
    std::vector<bool> is_inlier(total_points, false);
    for (uint32_t idx : inliers) is_inlier[idx] = true;
    std::vector<uint32_t> result;
    result.reserve(total_points - inliers.size());
    for (size_t i = 0; i < total_points; ++i)
      if (!is_inlier[i]) result.push_back(static_cast<uint32_t>(i));
    return result;
  }
  [[nodiscard]] bool success() const noexcept { return model.isValid() && !inliers.empty(); }
};

struct RansacConfig {  // ransac_plane.hpp:104-110
  float distance_threshold{0.1f};
  int max_iterations{1000};
  double probability{0.99};
  size_t min_inliers{3};
  bool refine_model{true};
};

struct GroundSegConfig {  // ground_seg.hpp:34-40
  float grid_resolution = 0.5f;
  float cell_percentile = 0.2f;
  float ground_thickness = 0.3f;
  float max_ground_height = 0.5f;
  size_t min_points_per_cell = 2;
};

struct GroundSegResult {  // ground_seg.hpp:49-68
  std::vector<uint32_t> ground;
  std::vector<uint32_t> obstacles;
  [[nodiscard]] bool empty() const noexcept { return ground.empty() && obstacles.empty(); }
  [[nodiscard]] float groundRatio() const noexcept {
    const size_t total = ground.size() + obstacles.size();
    return total > 0 ? static_cast<float>(ground.size()) / static_cast<float>(total) : 0.0f;
  }
};

namespace detail {
inline fdm_ransac_config to_abi(const RansacConfig& c) {
  fdm_ransac_config a{};
  a.distance_threshold = c.distance_threshold;
  a.max_iterations = c.max_iterations;
  a.probability = c.probability;
  a.min_inliers = c.min_inliers;
  a.refine_model = c.refine_model ? 1 : 0;
  return a;
}
inline RansacResult from_abi(const fdm_ransac_result& r, const uint32_t* inliers) {
  RansacResult out;
  out.model.coefficients = Point4(r.coefficients[0], r.coefficients[1], r.coefficients[2], r.coefficients[3]);
  out.inliers.assign(inliers, inliers + r.n_inliers);
  out.fitness = r.fitness;
  out.iterations = r.iterations;
  return out;
}
constexpr int kDevice = 0;
}  // namespace detail

[[nodiscard]] inline RansacResult segmentPlane(const PointCloud& cloud, const std::vector<uint32_t>& indices,
                                               const RansacConfig& config = RansacConfig{}) {
  if (indices.size() < 3) return {};  // ransac_plane_impl.hpp:247
  const fdm_ransac_config c = detail::to_abi(config);
  std::vector<uint32_t> inliers(indices.size());
  fdm_ransac_result r;
  const int rc = fdm_cloud_segment_plane(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, indices.data(),
                                         indices.size(), &c, detail::kDevice, inliers.data(), &r);
  if (rc < 0) throw std::runtime_error(std::string("segmentPlane: ") + fdm_last_error());
  return detail::from_abi(r, inliers.data());
}

[[nodiscard]] inline RansacResult segmentPlane(const PointCloud& cloud, float distance_threshold, int max_iterations = 1000,
                                               double probability = 0.99) {
  if (cloud.size() < 3) return {};  // ransac_plane_impl.hpp:345
  RansacConfig config;
  config.distance_threshold = distance_threshold;
  config.max_iterations = max_iterations;
  config.probability = probability;
  const fdm_ransac_config c = detail::to_abi(config);
  std::vector<uint32_t> inliers(cloud.size());
  fdm_ransac_result r;
  const int rc = fdm_cloud_segment_plane(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, nullptr, 0, &c,
                                         detail::kDevice, inliers.data(), &r);  // every point, in order (:349-352)
  if (rc < 0) throw std::runtime_error(std::string("segmentPlane: ") + fdm_last_error());
  return detail::from_abi(r, inliers.data());
}

[[nodiscard]] inline std::vector<RansacResult> segmentMultiplePlanes(const PointCloud& cloud,
                                                                     const RansacConfig& config = RansacConfig{},
                                                                     size_t max_planes = 5, double min_fitness = 0.1) {
  std::vector<RansacResult> results;
  if (cloud.size() < 3 || max_planes == 0) return results;
  const fdm_ransac_config c = detail::to_abi(config);
  std::vector<uint32_t> inliers(cloud.size());
  std::vector<fdm_ransac_result> rs(max_planes);
  uint64_t count = 0;
  const int rc = fdm_cloud_segment_planes(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, &c, max_planes,
                                          min_fitness, detail::kDevice, inliers.data(), rs.data(), &count);
  if (rc < 0) throw std::runtime_error(std::string("segmentMultiplePlanes: ") + fdm_last_error());
  results.reserve(count);
  const uint32_t* at = inliers.data();
  for (uint64_t k = 0; k < count; ++k) {
    results.push_back(detail::from_abi(rs[k], at));
    at += rs[k].n_inliers;
  }
  return results;
}

[[nodiscard]] inline GroundSegResult segmentGround(const PointCloud& cloud, const GroundSegConfig& config = GroundSegConfig{}) {
  GroundSegResult result;
  if (cloud.empty()) return result;  // ground_seg_impl.hpp:72-74
  fdm_ground_seg_config c{};
  c.grid_resolution = config.grid_resolution;
  c.cell_percentile = config.cell_percentile;
  c.ground_thickness = config.ground_thickness;
  c.max_ground_height = config.max_ground_height;
  c.min_points_per_cell = config.min_points_per_cell;
  result.ground.resize(cloud.size());
  result.obstacles.resize(cloud.size());
  uint64_t n_ground = 0, n_obstacles = 0;
  const int rc = fdm_cloud_segment_ground(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, &c, detail::kDevice,
                                          result.ground.data(), result.obstacles.data(), &n_ground, &n_obstacles);
  if (rc < 0) throw std::runtime_error(std::string("segmentGround: ") + fdm_last_error());
  result.ground.resize(n_ground);
  result.obstacles.resize(n_obstacles);
  return result;
}

[[nodiscard]] inline GroundSegResult segmentGround(const PointCloud& cloud, float grid_resolution,
                                                   float ground_thickness = 0.3f, float max_ground_height = 0.5f) {
  GroundSegConfig config;  // ground_seg_impl.hpp:114-123
  config.grid_resolution = grid_resolution;
  config.ground_thickness = ground_thickness;
  config.max_ground_height = max_ground_height;
  return segmentGround(cloud, config);
}

// the reference's Euclidean clustering (euclidean_cluster.hpp): not provided — see the head of this file
struct ClusterConfig;
struct ClusterResult;
ClusterResult euclideanCluster(const PointCloud& cloud, const ClusterConfig& config) = delete;

}  // namespace segmentation
}  // namespace nanopcl
