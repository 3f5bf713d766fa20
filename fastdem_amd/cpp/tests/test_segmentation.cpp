// test_segmentation.cpp — nanoPCL's segmentation tests (lib/nanoPCL/tests/test_segmentation.cpp): its RANSAC group
// (:283-376), its ground group (:382-498) and the RANSAC / ground parts of its boundary group (:511-549) at their own
// bounds, re-expressed on the mirror's nanopcl/segmentation.hpp.  The helper clouds are written anew: the reference's
// draw from rand(), these from a seeded generator, to the same construction.  The clustering cases have no counterpart
// (euclideanCluster is declared deleted).  Plus what the mirror adds: the result's helpers, an index out of range.
// Needs a device (tests/test_segmentation_cpp_gpu.py runs it).
#include <cmath>
#include <random>
#include <stdexcept>
#include <vector>

#include "mini_test.hpp"
#include "nanopcl/core.hpp"

using nanopcl::Point;
using nanopcl::PointCloud;
namespace segmentation = nanopcl::segmentation;

namespace {
struct Dice {  // a value in 0 .. 99, as the reference's rand() % 100
  std::mt19937 rng;
  explicit Dice(unsigned seed) : rng(seed) {}
  float operator()() { return float(rng() % 100u); }
};

// a flat ground at z = 0 with a little noise
PointCloud groundPlane(int nx, int ny, float spacing, float noise, unsigned seed) {
  Dice d(seed);
  PointCloud cloud;
  for (int x = 0; x < nx; ++x)
    for (int y = 0; y < ny; ++y) cloud.add(float(x) * spacing, float(y) * spacing, d() * noise * 0.01f);
  return cloud;
}
// `per` points in every cell of an nx x ny block of unit cells starting at x0, all at height z
void addDenseLayer(PointCloud& cloud, Dice& d, int nx, int ny, int per, float z, float x0 = 0.0f) {
  for (int x = 0; x < nx; ++x)
    for (int y = 0; y < ny; ++y)
      for (int k = 0; k < per; ++k) cloud.add(x0 + float(x) + d() * 0.004f, float(y) + d() * 0.004f, z);
}
// dense ground on the 0.5 m grid and two obstacles above it
PointCloud groundWithObstacles(unsigned seed) {
  Dice d(seed);
  PointCloud cloud;
  for (int x = -10; x <= 10; ++x)
    for (int y = -10; y <= 10; ++y)
      for (int k = 0; k < 3; ++k) cloud.add(float(x) * 0.5f + d() * 0.004f, float(y) * 0.5f + d() * 0.004f, d() * 0.001f);
  for (int i = 0; i < 40; ++i) cloud.add(2.0f + d() * 0.005f, 2.0f + d() * 0.005f, 1.0f + d() * 0.01f);
  for (int i = 0; i < 40; ++i) cloud.add(-2.0f + d() * 0.005f, -2.0f + d() * 0.005f, 1.0f + d() * 0.01f);
  return cloud;
}
PointCloud grid(std::initializer_list<float> heights) {
  PointCloud cloud;
  for (float z : heights)
    for (int x = 0; x < 10; ++x)
      for (int y = 0; y < 10; ++y) cloud.add(float(x), float(y), z);
  return cloud;
}
}  // namespace

// ---- RANSAC (:283-376) ----
TEST(Ransac, plane_detection) {
  const PointCloud cloud = groundPlane(20, 20, 0.5f, 0.01f, 1);
  const auto result = segmentation::segmentPlane(cloud, 0.05f);
  EXPECT_TRUE(result.success());
  EXPECT_GT(result.fitness, 0.9);
}

TEST(Ransac, plane_model_accuracy) {
  const PointCloud cloud = grid({1.0f});
  const auto result = segmentation::segmentPlane(cloud, 0.1f);
  ASSERT_TRUE(result.success());
  EXPECT_NEAR(std::abs(result.model.coefficients.z()), 1.0f, 0.01f);
  EXPECT_NEAR(std::abs(result.model.coefficients.w()), 1.0f, 0.1f);
}

TEST(Ransac, inlier_outlier_split) {
  PointCloud cloud = groundPlane(10, 10, 1.0f, 0.01f, 2);
  const size_t ground_size = cloud.size();
  for (int i = 0; i < 20; ++i) cloud.add(float(i % 10), float(i / 10), 5.0f);
  const auto result = segmentation::segmentPlane(cloud, 0.1f);
  const auto outliers = result.outliers(cloud.size());
  EXPECT_TRUE(result.success());
  EXPECT_GE(double(result.inliers.size()), double(ground_size) * 0.9);
  EXPECT_GE(outliers.size(), size_t(15));
  EXPECT_EQ(result.inliers.size() + outliers.size(), cloud.size());
}

TEST(Ransac, multiple_planes) {
  const PointCloud cloud = grid({0.0f, 5.0f});
  segmentation::RansacConfig config;
  config.distance_threshold = 0.1f;
  config.max_iterations = 500;
  const auto results = segmentation::segmentMultiplePlanes(cloud, config, 3, 0.1);
  ASSERT_TRUE(results.size() >= 2);
  EXPECT_EQ(results[0].inliers.size(), size_t(100));
  EXPECT_EQ(results[1].inliers.size(), size_t(100));
}

TEST(Ransac, collinear_points) {
  PointCloud cloud;
  for (int i = 0; i < 10; ++i) cloud.add(float(i), 0, 0);
  const auto result = segmentation::segmentPlane(cloud, 0.1f, 100);
  EXPECT_TRUE(result.inliers.size() <= cloud.size());
  EXPECT_FALSE(result.success());  // every sample is collinear: the default result
  EXPECT_EQ(result.iterations, 0);
}

TEST(Ransac, plane_from_points) {
  const auto model = segmentation::PlaneModel::fromPoints(Point(0, 0, 0), Point(1, 0, 0), Point(0, 1, 0));
  EXPECT_TRUE(model.isValid());
  EXPECT_NEAR(std::abs(model.coefficients.z()), 1.0f, 0.01f);
  EXPECT_NEAR(model.coefficients.w(), 0.0f, 0.01f);
  EXPECT_NEAR(model.distance(Point(3, 4, -2)), 2.0f, 1e-6f);
  EXPECT_NEAR(std::abs(model.signedDistance(Point(3, 4, -2))), 2.0f, 1e-6f);
  EXPECT_FALSE(segmentation::PlaneModel::fromPoints(Point(0, 0, 0), Point(1, 0, 0), Point(2, 0, 0)).isValid());
}

// ---- ground (:382-498) ----
TEST(Ground, basic_segmentation) {
  const PointCloud cloud = groundWithObstacles(3);
  const auto result = segmentation::segmentGround(cloud, 0.5f, 0.3f, 0.5f);
  EXPECT_FALSE(result.empty());
  EXPECT_GT(result.ground.size(), size_t(0));
  EXPECT_GT(result.obstacles.size(), size_t(0));
  EXPECT_EQ(result.ground.size() + result.obstacles.size(), cloud.size());
}

TEST(Ground, grid_resolution) {
  Dice d(4);
  PointCloud cloud;
  for (int x = 0; x < 20; ++x)
    for (int y = 0; y < 20; ++y)
      for (int k = 0; k < 3; ++k) cloud.add(float(x) * 0.5f + d() * 0.004f, float(y) * 0.5f + d() * 0.004f, d() * 0.001f);
  for (int i = 0; i < 20; ++i) cloud.add(5.0f, 5.0f, 1.0f + float(i) * 0.05f);
  EXPECT_GT(segmentation::segmentGround(cloud, 0.5f).ground.size(), size_t(0));
  EXPECT_GT(segmentation::segmentGround(cloud, 2.0f).ground.size(), size_t(0));
}

TEST(Ground, thickness_config) {
  Dice d(5);
  PointCloud cloud;
  addDenseLayer(cloud, d, 10, 5, 5, 0.0f);
  addDenseLayer(cloud, d, 10, 5, 3, 0.2f);
  segmentation::GroundSegConfig thin, thick;
  thin.ground_thickness = 0.1f;
  thin.grid_resolution = 1.0f;
  thick.ground_thickness = 0.5f;
  thick.grid_resolution = 1.0f;
  EXPECT_GT(segmentation::segmentGround(cloud, thick).ground.size(), segmentation::segmentGround(cloud, thin).ground.size());
}

TEST(Ground, height_config) {
  Dice d(6);
  PointCloud cloud;
  addDenseLayer(cloud, d, 10, 5, 3, 0.0f);
  addDenseLayer(cloud, d, 10, 5, 3, 1.0f, 20.0f);
  segmentation::GroundSegConfig config;
  config.max_ground_height = 0.5f;
  config.grid_resolution = 1.0f;
  const auto result = segmentation::segmentGround(cloud, config);
  EXPECT_EQ(result.ground.size(), size_t(150));     // the low layer
  EXPECT_EQ(result.obstacles.size(), size_t(150));  // the cells whose robust minimum is above max_ground_height
  EXPECT_NEAR(result.groundRatio(), 0.5f, 1e-6f);
}

// ---- boundaries (:511-549) ----
TEST(Boundary, empty_cloud_ransac) {
  const PointCloud empty;
  EXPECT_FALSE(segmentation::segmentPlane(empty, 0.1f).success());
  EXPECT_TRUE(segmentation::segmentMultiplePlanes(empty).empty());
}

TEST(Boundary, empty_cloud_ground) {
  const PointCloud empty;
  const auto result = segmentation::segmentGround(empty);
  EXPECT_TRUE(result.empty());
  EXPECT_EQ(result.groundRatio(), 0.0f);
}

TEST(Boundary, single_point) {
  PointCloud single;
  single.add(1.0f, 2.0f, 3.0f);
  EXPECT_FALSE(segmentation::segmentPlane(single, 0.1f).success());
  const auto ground = segmentation::segmentGround(single);
  EXPECT_EQ(ground.ground.size() + ground.obstacles.size(), size_t(1));
}

TEST(Boundary, insufficient_points_for_plane) {
  PointCloud cloud;
  cloud.add(0, 0, 0);
  cloud.add(1, 0, 0);
  EXPECT_FALSE(segmentation::segmentPlane(cloud, 0.1f).success());
}

// ---- the mirror's own ----
TEST(Mirror, index_list_and_errors) {
  const PointCloud cloud = grid({0.0f, 5.0f});
  std::vector<uint32_t> upper;
  for (uint32_t i = 100; i < 200; ++i) upper.push_back(i);
  const auto result = segmentation::segmentPlane(cloud, upper);
  ASSERT_TRUE(result.success());
  EXPECT_EQ(result.inliers.size(), size_t(100));
  EXPECT_EQ(result.inliers.front(), 100u);
  EXPECT_NEAR(std::abs(result.model.coefficients.w()), 5.0f, 1e-4f);
  EXPECT_EQ(result.fitness, 1.0);
  upper[5] = 200;  // not a point of the cloud
  EXPECT_THROW((void)segmentation::segmentPlane(cloud, upper), std::runtime_error);
  EXPECT_THROW((void)segmentation::segmentGround(cloud, -1.0f), std::runtime_error);
  const segmentation::RansacResult none;
  EXPECT_FALSE(none.success());
  EXPECT_EQ(none.model.coefficients.z(), 1.0f);
  EXPECT_EQ(none.outliers(3).size(), size_t(3));
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
