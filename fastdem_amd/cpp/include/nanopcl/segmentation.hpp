// nanopcl/segmentation.hpp — nanopcl::segmentation::segmentGround, segmentPlane and segmentMultiplePlanes of the reference
// (lib/nanoPCL/include/nanopcl/segmentation/ground_seg.hpp:34-106, ransac_plane.hpp:41-158) over
// fdm_cloud_segment_ground / _plane / _planes: the cloud's x, y, z channels go to the device as they are, the cells'
// sorts and the hypotheses' scoring run there (include/fdm_engine.h states what is computed, the refinement's summation
// order and the refined normal's sign included).  Names, signatures and defaults are the reference's.  PlaneModel's own
// arithmetic (fromPoints, signedDistance, distance, isValid) runs on the host, in the order the header states.
//
// euclideanCluster, ClusterConfig, ClusterResult and applyClusterLabels (segmentation/euclidean_cluster.hpp) over
// fdm_cloud_cluster: the clusters are the reference's — the connected components of its radius relation, filtered by size —
// in THIS PROJECT'S order: descending size, equal sizes by their smallest member's list position, members in ascending
// list position (the reference's final std::sort read as a stable one; its BFS order inside a cluster is not reproduced).
#pragma once
#include <algorithm>
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

// ---- Euclidean clustering (segmentation/euclidean_cluster.hpp) ----
struct ClusterConfig {
  float tolerance = 0.5f;    // distance threshold for neighbours
  size_t min_size = 10;      // points a cluster has at least
  size_t max_size = 100000;  // ... and at most: a larger component is dropped whole
};

struct ClusterResult {  // CSR: all clustered point indices, and where each cluster starts
  std::vector<uint32_t> indices;
  std::vector<uint32_t> offsets;  // [0, n0, n0 + n1, ...]

  [[nodiscard]] size_t numClusters() const noexcept { return offsets.empty() ? 0 : offsets.size() - 1; }
  [[nodiscard]] size_t clusterSize(size_t i) const noexcept { return offsets[i + 1] - offsets[i]; }
  [[nodiscard]] size_t totalClusteredPoints() const noexcept { return indices.size(); }
  [[nodiscard]] bool empty() const noexcept { return numClusters() == 0; }
  [[nodiscard]] Span<const uint32_t> clusterIndices(size_t i) const {
    return Span<const uint32_t>(indices.data() + offsets[i], offsets[i + 1] - offsets[i]);
  }
  // cluster i as a cloud of its own, every channel of `cloud` kept
  [[nodiscard]] PointCloud extract(const PointCloud& cloud, size_t i) const {
    const Span<const uint32_t> members = clusterIndices(i);
    return cloud.extract(std::vector<size_t>(members.begin(), members.end()));
  }
  // the indices 0 .. total_points - 1 that are in no cluster, ascending
  [[nodiscard]] std::vector<uint32_t> noiseIndices(size_t total_points) const {
    std::vector<bool> clustered(total_points, false);
    for (uint32_t idx : indices) clustered[idx] = true;
    std::vector<uint32_t> noise;
    noise.reserve(total_points - std::min(total_points, indices.size()));
    for (size_t i = 0; i < total_points; ++i)
      if (!clustered[i]) noise.push_back(static_cast<uint32_t>(i));
    return noise;
  }
  [[nodiscard]] std::vector<size_t> clusterSizes() const {
    std::vector<size_t> sizes(numClusters());
    for (size_t i = 0; i < sizes.size(); ++i) sizes[i] = clusterSize(i);
    return sizes;
  }
};

namespace detail {
// indices NULL: every point of the cloud, in order
inline ClusterResult cluster(const PointCloud& cloud, const uint32_t* indices, size_t count, const ClusterConfig& config) {
  ClusterResult result;
  if (count == 0) {  // an empty cloud or list: one offset, no device call
    result.offsets.push_back(0);
    return result;
  }
  fdm_cluster_config c{};
  c.tolerance = config.tolerance;
  c.min_size = config.min_size;
  c.max_size = config.max_size;
  result.indices.resize(count);
  result.offsets.resize(count + 1);
  uint64_t n_clusters = 0;
  const int rc = fdm_cloud_cluster(cloud.size(), cloud.xData(), cloud.yData(), cloud.zData(), 0, indices, count, &c,
                                   kDevice, result.indices.data(), result.offsets.data(), nullptr, &n_clusters);
  if (rc < 0) throw std::runtime_error(std::string("euclideanCluster: ") + fdm_last_error());
  result.offsets.resize(n_clusters + 1);
  result.indices.resize(result.offsets.back());
  return result;
}
}  // namespace detail

[[nodiscard]] inline ClusterResult euclideanCluster(const PointCloud& cloud, const ClusterConfig& config = ClusterConfig{}) {
  return detail::cluster(cloud, nullptr, cloud.size(), config);
}
[[nodiscard]] inline ClusterResult euclideanCluster(const PointCloud& cloud, float tolerance, size_t min_size = 10,
                                                    size_t max_size = 100000) {
  return euclideanCluster(cloud, ClusterConfig{tolerance, min_size, max_size});
}
// over a subset of the cloud: the returned indices are the list's entries, i.e. they reference `cloud`
[[nodiscard]] inline ClusterResult euclideanCluster(const PointCloud& cloud, const std::vector<uint32_t>& subset_indices,
                                                    const ClusterConfig& config = ClusterConfig{}) {
  return detail::cluster(cloud, subset_indices.data(), subset_indices.size(), config);
}
[[nodiscard]] inline ClusterResult euclideanCluster(const PointCloud& cloud, const std::vector<uint32_t>& subset_indices,
                                                    float tolerance, size_t min_size = 10, size_t max_size = 100000) {
  return euclideanCluster(cloud, subset_indices, ClusterConfig{tolerance, min_size, max_size});
}

// the Label channel from a clustering: instance id = cluster number + 1 (16 bits, truncated), 0 for noise; the semantic
// class in the upper 16 bits.  Labels the cloud already has are overwritten.
inline void applyClusterLabels(PointCloud& cloud, const ClusterResult& result, uint16_t semantic_class = 0) {
  cloud.useLabel();
  const uint32_t upper = static_cast<uint32_t>(semantic_class) << 16;
  for (Label& l : cloud.labels()) l = Label(upper);
  for (size_t k = 0; k < result.numClusters(); ++k) {
    const Label mark(upper | static_cast<uint16_t>(k + 1));
    for (uint32_t idx : result.clusterIndices(k)) cloud.labels()[idx] = mark;
  }
}

}  // namespace segmentation
}  // namespace nanopcl
