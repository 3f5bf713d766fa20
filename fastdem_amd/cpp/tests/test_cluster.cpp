// test_cluster.cpp — the clustering cases of nanoPCL's segmentation tests (lib/nanoPCL/tests/test_segmentation.cpp: its
// Euclidean group :111-277, the clustering parts of its boundary group :504-531, its channel test :555-584 and its two
// pipeline tests :590-627) at their own bounds, re-expressed on the mirror's nanopcl/segmentation.hpp.  The helper clouds
// are written anew: the reference's draw from rand(), these from a seeded generator, to the same construction.  Plus
// what the mirror states beyond the reference: the four overloads agree, the order of clusters and members, the refusals.
// Needs a device (tests/test_cluster_cpp_gpu.py runs it).
#include <algorithm>
#include <cmath>
#include <limits>
#include <random>
#include <stdexcept>
#include <vector>

#include "mini_test.hpp"
#include "nanopcl/core.hpp"

using nanopcl::Color;
using nanopcl::Intensity;
using nanopcl::PointCloud;
namespace segmentation = nanopcl::segmentation;

namespace {
struct Dice {  // a value in 0 .. 99, as the reference's rand() % 100
  std::mt19937 rng;
  explicit Dice(unsigned seed) : rng(seed) {}
  float operator()() { return float(rng() % 100u); }
};

// three separate groups of 50, 30 and 20 points, each inside a 0.5 m cube
PointCloud threeGroups(unsigned seed) {
  Dice d(seed);
  PointCloud cloud;
  const float cx[3] = {0.0f, 5.0f, 0.0f}, cy[3] = {0.0f, 0.0f, 5.0f};
  const int count[3] = {50, 30, 20};
  for (int g = 0; g < 3; ++g)
    for (int i = 0; i < count[g]; ++i) cloud.add(cx[g] + d() * 0.005f, cy[g] + d() * 0.005f, 1.0f + d() * 0.005f);
  return cloud;
}
// dense ground on the 0.5 m grid and two obstacles of 40 points above it
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
segmentation::ClusterConfig config(float tolerance, size_t min_size, size_t max_size = 100000) {
  segmentation::ClusterConfig c;
  c.tolerance = tolerance;
  c.min_size = min_size;
  c.max_size = max_size;
  return c;
}
}  // namespace

// ---- Euclidean clustering (:111-277) ----
TEST(Euclidean, basic_clustering) {
  const PointCloud cloud = threeGroups(1);
  ASSERT_EQ(cloud.size(), 100u);
  const auto result = segmentation::euclideanCluster(cloud, config(1.0f, 10, 100));
  ASSERT_EQ(result.numClusters(), 3u);
  ASSERT_EQ(result.totalClusteredPoints(), 100u);
}

TEST(Euclidean, csr_format) {
  const PointCloud cloud = threeGroups(2);
  const auto result = segmentation::euclideanCluster(cloud, config(1.0f, 10));
  ASSERT_EQ(result.offsets.size(), result.numClusters() + 1);
  ASSERT_EQ(result.offsets[0], 0u);
  size_t total = 0;
  for (size_t i = 0; i < result.numClusters(); ++i) total += result.clusterSize(i);
  ASSERT_EQ(total, result.totalClusteredPoints());
  const std::vector<size_t> want = {50, 30, 20};  // largest first
  EXPECT_TRUE(result.clusterSizes() == want);
}

TEST(Euclidean, cluster_extraction) {
  const PointCloud cloud = threeGroups(3);
  const auto result = segmentation::euclideanCluster(cloud, config(1.0f, 10));
  ASSERT_TRUE(result.numClusters() >= 1);
  const PointCloud cluster0 = result.extract(cloud, 0);
  ASSERT_EQ(cluster0.size(), result.clusterSize(0));
  for (size_t i = 0; i < cluster0.size(); ++i) ASSERT_TRUE(std::isfinite(cluster0.point(i).x()));
}

TEST(Euclidean, config_tolerance) {
  PointCloud cloud;
  for (int i = 0; i < 20; ++i) {
    cloud.add(float(i) * 0.1f, 0, 0);
    cloud.add(10.0f + float(i) * 0.1f, 0, 0);
  }
  ASSERT_EQ(segmentation::euclideanCluster(cloud, config(0.5f, 5)).numClusters(), 2u);
  ASSERT_EQ(segmentation::euclideanCluster(cloud, 0.5f, 5).numClusters(), 2u);
}

TEST(Euclidean, config_min_max_size) {
  const PointCloud cloud = threeGroups(4);
  ASSERT_EQ(segmentation::euclideanCluster(cloud, config(1.0f, 25, 100)).numClusters(), 2u);  // 20 is too few
  const auto capped = segmentation::euclideanCluster(cloud, config(1.0f, 10, 40));            // 50 is dropped whole
  ASSERT_EQ(capped.numClusters(), 2u);
  EXPECT_EQ(capped.totalClusteredPoints(), 50u);
}

TEST(Euclidean, subset_clustering) {
  const PointCloud cloud = groundWithObstacles(5);
  std::vector<uint32_t> subset;
  for (size_t i = 0; i < cloud.size(); ++i)
    if (cloud.point(i).z() > 0.5f) subset.push_back(static_cast<uint32_t>(i));
  const auto result = segmentation::euclideanCluster(cloud, subset, config(0.5f, 10));
  EXPECT_GE(result.numClusters(), 1u);
  for (size_t i = 0; i < result.numClusters(); ++i)
    for (uint32_t idx : result.clusterIndices(i)) {
      EXPECT_LT(idx, cloud.size());
      EXPECT_TRUE(cloud.point(idx).z() > 0.5f);  // an entry of the list, not a position in it
    }
}

TEST(Euclidean, apply_labels) {
  PointCloud cloud = threeGroups(6);
  const auto result = segmentation::euclideanCluster(cloud, config(1.0f, 10));
  segmentation::applyClusterLabels(cloud, result, 1);
  ASSERT_TRUE(cloud.hasLabel());
  ASSERT_EQ(cloud.labels().size(), cloud.size());
  size_t labeled = 0;
  for (size_t i = 0; i < cloud.size(); ++i) {
    if ((cloud.label(i).val & 0xFFFF) > 0) ++labeled;
    EXPECT_EQ(cloud.label(i).val >> 16, 1u);
  }
  ASSERT_EQ(labeled, result.totalClusteredPoints());
  for (uint32_t idx : result.clusterIndices(1)) EXPECT_EQ(cloud.label(idx).instanceId(), 2u);
}

TEST(Euclidean, noise_indices) {
  PointCloud cloud;
  for (int i = 0; i < 50; ++i) cloud.add(float(i) * 0.1f, 0, 0);
  cloud.add(100.0f, 0, 0);
  cloud.add(200.0f, 0, 0);
  const auto result = segmentation::euclideanCluster(cloud, config(0.5f, 10));
  const auto noise = result.noiseIndices(cloud.size());
  ASSERT_EQ(noise.size(), 2u);
  EXPECT_EQ(noise[0], 50u);
  EXPECT_EQ(noise[1], 51u);
}

// ---- boundary conditions (:504-531) ----
TEST(Boundary, empty_cloud_clustering) {
  const PointCloud empty;
  const auto result = segmentation::euclideanCluster(empty);
  ASSERT_EQ(result.numClusters(), 0u);
  ASSERT_TRUE(result.empty());
  EXPECT_EQ(result.offsets.size(), 1u);
  const auto none = segmentation::euclideanCluster(threeGroups(7), std::vector<uint32_t>{});
  EXPECT_TRUE(none.empty());
  EXPECT_EQ(none.offsets.size(), 1u);
}

TEST(Boundary, single_point_clustering) {
  PointCloud single;
  single.add(1.0f, 2.0f, 3.0f);
  segmentation::ClusterConfig c;
  c.min_size = 2;
  ASSERT_EQ(segmentation::euclideanCluster(single, c).numClusters(), 0u);
  c.min_size = 1;
  ASSERT_EQ(segmentation::euclideanCluster(single, c).numClusters(), 1u);
}

// ---- channels (:555-584) ----
TEST(Channels, cluster_extract_preserves_channels) {
  PointCloud cloud;
  cloud.useIntensity();
  cloud.useColor();
  for (int i = 0; i < 20; ++i) {
    cloud.add(float(i) * 0.1f, 0, 0, Intensity(0.5f));
    cloud.setColor(cloud.size() - 1, Color(100, 150, 200));
  }
  for (int i = 0; i < 20; ++i) {
    cloud.add(10.0f + float(i) * 0.1f, 0, 0, Intensity(0.8f));
    cloud.setColor(cloud.size() - 1, Color(50, 100, 150));
  }
  const auto result = segmentation::euclideanCluster(cloud, config(0.5f, 10));
  ASSERT_EQ(result.numClusters(), 2u);
  const PointCloud extracted = result.extract(cloud, 0);
  ASSERT_TRUE(extracted.hasIntensity());
  ASSERT_TRUE(extracted.hasColor());
  ASSERT_EQ(extracted.size(), result.clusterSize(0));
  // equal sizes: the cluster of the smaller first index comes first, its members in ascending index
  for (size_t i = 0; i < extracted.size(); ++i) {
    EXPECT_EQ(result.clusterIndices(0)[i], uint32_t(i));
    EXPECT_FLOAT_EQ(extracted.intensity(i), 0.5f);
    EXPECT_EQ(int(extracted.color(i).g), 150);
    EXPECT_FLOAT_EQ(extracted.point(i).x(), float(i) * 0.1f);
  }
}

// ---- pipelines (:590-627) ----
TEST(Integration, ground_removal_then_clustering) {
  const PointCloud cloud = groundWithObstacles(8);
  const auto ground = segmentation::segmentGround(cloud, 0.5f, 0.3f, 0.5f);
  const auto clusters = segmentation::euclideanCluster(cloud, ground.obstacles, config(0.5f, 10));
  EXPECT_GE(clusters.numClusters(), 1u);
  EXPECT_LE(clusters.totalClusteredPoints(), ground.obstacles.size());
}

TEST(Integration, ransac_then_clustering) {
  const PointCloud cloud = groundWithObstacles(9);
  const auto plane = segmentation::segmentPlane(cloud, 0.1f);
  ASSERT_TRUE(plane.success());
  const auto clusters = segmentation::euclideanCluster(cloud, plane.outliers(cloud.size()), config(0.5f, 10));
  EXPECT_GE(clusters.numClusters(), 1u);
}

// ---- what the mirror states beyond the reference ----
TEST(Mirror, overloads_agree_and_order_is_stated) {
  const PointCloud cloud = threeGroups(10);
  std::vector<uint32_t> all(cloud.size());
  for (size_t i = 0; i < all.size(); ++i) all[i] = uint32_t(i);
  const auto a = segmentation::euclideanCluster(cloud, config(1.0f, 10, 100));
  const auto b = segmentation::euclideanCluster(cloud, 1.0f, 10, 100);
  const auto c = segmentation::euclideanCluster(cloud, all, config(1.0f, 10, 100));
  const auto d = segmentation::euclideanCluster(cloud, all, 1.0f, 10, 100);
  EXPECT_TRUE(a.indices == b.indices && a.indices == c.indices && a.indices == d.indices);
  EXPECT_TRUE(a.offsets == b.offsets && a.offsets == c.offsets && a.offsets == d.offsets);
  for (size_t k = 0; k < a.numClusters(); ++k) {
    const auto m = a.clusterIndices(k);
    EXPECT_TRUE(std::is_sorted(m.begin(), m.end()));
    if (k) EXPECT_GE(a.clusterSize(k - 1), a.clusterSize(k));
  }
  // a reversed list: positions ascend inside a cluster, so the entries descend
  std::vector<uint32_t> reversed(all.rbegin(), all.rend());
  const auto r = segmentation::euclideanCluster(cloud, reversed, config(1.0f, 10, 100));
  ASSERT_EQ(r.numClusters(), 3u);
  const auto m0 = r.clusterIndices(0);
  EXPECT_TRUE(std::is_sorted(m0.begin(), m0.end(), [](uint32_t p, uint32_t q) { return p > q; }));
  EXPECT_EQ(r.clusterSize(0), 50u);
}

TEST(Mirror, refusals) {
  PointCloud cloud = threeGroups(11);
  EXPECT_THROW((void)segmentation::euclideanCluster(cloud, 0.0f), std::runtime_error);
  EXPECT_THROW((void)segmentation::euclideanCluster(cloud, -1.0f), std::runtime_error);
  EXPECT_THROW((void)segmentation::euclideanCluster(cloud, std::numeric_limits<float>::quiet_NaN()), std::runtime_error);
  EXPECT_THROW((void)segmentation::euclideanCluster(cloud, std::vector<uint32_t>{0u, 100u}), std::runtime_error);
  cloud.point(3) = Eigen::Vector3f(std::numeric_limits<float>::quiet_NaN(), 0.0f, 0.0f);
  EXPECT_THROW((void)segmentation::euclideanCluster(cloud), std::runtime_error);
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
