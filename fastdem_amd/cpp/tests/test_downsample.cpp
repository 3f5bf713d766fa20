// test_downsample.cpp — nanoPCL's voxelGrid and gridMaxZ tests (lib/nanoPCL/tests/test_filters.cpp:159-317, and the
// filters' share of its empty-cloud, single-point and NaN cases at :786-812) re-expressed on the mirror's
// nanopcl/filters/downsample.hpp, plus what the mirror adds: the channel layout and metadata of the output, the refused
// sizes, the process-wide order.  Needs a device: the filters run there (tests/test_downsample_cpp_gpu.py runs it).
#include <cmath>
#include <limits>
#include <stdexcept>

#include "mini_test.hpp"
#include "nanopcl/filters/downsample.hpp"

using nanopcl::Color;
using nanopcl::Intensity;
using nanopcl::Normal4;
using nanopcl::PointCloud;
namespace filters = nanopcl::filters;

static PointCloud createGrid3x3x3() {
  PointCloud cloud;
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < 3; ++y)
      for (int z = 0; z < 3; ++z) cloud.add(float(x), float(y), float(z));
  return cloud;
}

TEST(VoxelGrid, centroid) {
  PointCloud cloud;
  cloud.add(0.0f, 0.0f, 0.0f);
  cloud.add(1.0f, 0.0f, 0.0f);
  cloud.add(0.0f, 1.0f, 0.0f);
  cloud.add(1.0f, 1.0f, 0.0f);
  auto downsampled = filters::voxelGrid(cloud, 2.0f, filters::VoxelMode::CENTROID);
  ASSERT_EQ(downsampled.size(), 1u);
  EXPECT_NEAR(downsampled.point(0).x(), 0.5f, 0.01f);
  EXPECT_NEAR(downsampled.point(0).y(), 0.5f, 0.01f);
  EXPECT_NEAR(downsampled.point(0).z(), 0.0f, 0.01f);
}

TEST(VoxelGrid, nearest) {
  PointCloud cloud;
  cloud.add(0.1f, 0.1f, 0.0f);
  cloud.add(0.9f, 0.1f, 0.0f);
  cloud.add(0.1f, 0.9f, 0.0f);
  cloud.add(0.5f, 0.5f, 0.0f);  // closest to the centre (0.5, 0.5, 0.5)
  auto downsampled = filters::voxelGrid(cloud, 1.0f, filters::VoxelMode::NEAREST);
  ASSERT_EQ(downsampled.size(), 1u);
  EXPECT_NEAR(downsampled.point(0).x(), 0.5f, 0.01f);
  EXPECT_NEAR(downsampled.point(0).y(), 0.5f, 0.01f);
}

TEST(VoxelGrid, channel_averaging) {
  PointCloud cloud;
  cloud.useIntensity();
  cloud.add(0.0f, 0.0f, 0.0f);
  cloud.intensity(0) = 0.2f;
  cloud.add(0.5f, 0.5f, 0.0f);
  cloud.intensity(1) = 0.8f;
  auto downsampled = filters::voxelGrid(cloud, 1.0f, filters::VoxelMode::CENTROID);
  ASSERT_EQ(downsampled.size(), 1u);
  ASSERT_TRUE(downsampled.hasIntensity());
  EXPECT_NEAR(downsampled.intensity(0), 0.5f, 0.01f);
}

TEST(VoxelGrid, move_semantics) {
  PointCloud cloud = createGrid3x3x3();
  const size_t original_size = cloud.size();
  auto downsampled = filters::voxelGrid(std::move(cloud), 1.5f);
  EXPECT_TRUE(downsampled.size() < original_size);
  EXPECT_TRUE(downsampled.size() > 0);
  EXPECT_EQ(downsampled.size(), 8u);
}

TEST(VoxelGrid, covariance_preservation) {
  PointCloud cloud;
  cloud.useCovariance();
  cloud.add(0.0f, 0.0f, 0.0f);
  cloud.add(0.5f, 0.5f, 0.0f);
  for (int d = 0; d < 3; ++d) {
    cloud.covarianceData()[0 * 9 + d * 4] = 2.0f;
    cloud.covarianceData()[1 * 9 + d * 4] = 4.0f;
  }
  auto downsampled = filters::voxelGrid(cloud, 1.0f, filters::VoxelMode::CENTROID);
  ASSERT_EQ(downsampled.size(), 1u);
  ASSERT_TRUE(downsampled.hasCovariance());
  EXPECT_NEAR(downsampled.covariance(0)(0, 0), 2.0f, 0.01f);  // the representative's: the first point's
  EXPECT_NEAR(downsampled.covariance(0)(2, 2), 2.0f, 0.01f);
  EXPECT_NEAR(downsampled.covariance(0)(0, 1), 0.0f, 0.01f);
}

TEST(VoxelGrid, symmetry) {
  PointCloud cloud;
  for (float x = -10.0f; x <= 10.0f; x += 0.3f)
    for (float y = -10.0f; y <= 10.0f; y += 0.3f) cloud.add(x, y, 0.0f);
  size_t orig_neg_x = 0;
  for (size_t i = 0; i < cloud.size(); ++i)
    if (cloud.point(i).x() < 0) orig_neg_x++;
  auto downsampled = filters::voxelGrid(cloud, 0.3f);
  size_t down_neg_x = 0;
  for (size_t i = 0; i < downsampled.size(); ++i)
    if (downsampled.point(i).x() < 0) down_neg_x++;
  const float orig_ratio = static_cast<float>(orig_neg_x) / cloud.size();
  const float down_ratio = static_cast<float>(down_neg_x) / downsampled.size();
  EXPECT_TRUE(std::abs(orig_ratio - down_ratio) < 0.05f);
  EXPECT_TRUE(down_ratio > 0.45f && down_ratio < 0.55f);
}

TEST(GridMaxZ, basic) {
  PointCloud cloud;
  cloud.add(0.0f, 0.0f, 1.0f);
  cloud.add(0.0f, 0.0f, 5.0f);  // max
  cloud.add(0.0f, 0.0f, 3.0f);
  auto result = filters::gridMaxZ(cloud, 1.0f);
  ASSERT_EQ(result.size(), 1u);
  EXPECT_NEAR(result.point(0).z(), 5.0f, 0.01f);
}

TEST(GridMaxZ, multiple_cells) {
  PointCloud cloud;
  cloud.add(0.0f, 0.0f, 1.0f);
  cloud.add(0.0f, 0.0f, 3.0f);  // max of cell (0, 0)
  cloud.add(2.0f, 0.0f, 5.0f);  // max of cell (2, 0)
  cloud.add(2.0f, 0.0f, 2.0f);
  auto result = filters::gridMaxZ(cloud, 1.0f);
  ASSERT_EQ(result.size(), 2u);
  EXPECT_NEAR(result.point(0).z(), 3.0f, 0.01f);
  EXPECT_NEAR(result.point(1).z(), 5.0f, 0.01f);
}

TEST(GridMaxZ, channel_preservation) {
  PointCloud cloud;
  cloud.useIntensity();
  cloud.add(0.0f, 0.0f, 1.0f);
  cloud.intensity(0) = 0.1f;
  cloud.add(0.0f, 0.0f, 5.0f);  // max z
  cloud.intensity(1) = 0.9f;
  auto result = filters::gridMaxZ(cloud, 1.0f);
  ASSERT_EQ(result.size(), 1u);
  ASSERT_TRUE(result.hasIntensity());
  EXPECT_NEAR(result.intensity(0), 0.9f, 0.01f);
}

TEST(EdgeCases, empty_cloud) {
  PointCloud empty;
  auto voxelized = filters::voxelGrid(empty, 1.0f);
  EXPECT_TRUE(voxelized.empty());
  auto maxz = filters::gridMaxZ(empty, 1.0f);
  EXPECT_TRUE(maxz.empty());
  EXPECT_TRUE(filters::voxelGrid(PointCloud(), 1.0f).empty());
  EXPECT_TRUE(filters::gridMaxZ(PointCloud(), 1.0f).empty());
}

TEST(EdgeCases, single_point) {
  PointCloud single;
  single.add(1.0f, 2.0f, 3.0f);
  auto voxelized = filters::voxelGrid(single, 1.0f);
  ASSERT_EQ(voxelized.size(), 1u);
  auto maxz = filters::gridMaxZ(single, 1.0f);
  ASSERT_EQ(maxz.size(), 1u);
  EXPECT_EQ(maxz.point(0).z(), 3.0f);
}

TEST(EdgeCases, nan_handling_in_voxelGrid) {
  PointCloud cloud;
  cloud.add(1.0f, 2.0f, 3.0f);
  cloud.add(std::numeric_limits<float>::quiet_NaN(), 0, 0);
  cloud.add(4.0f, 5.0f, 6.0f);
  auto voxelized = filters::voxelGrid(cloud, 10.0f);
  ASSERT_EQ(voxelized.size(), 1u);  // the NaN point is skipped, the others merge
  EXPECT_EQ(voxelized.point(0).x(), 2.5f);
}

// ---- the mirror's own ----
TEST(Mirror, layout_metadata_and_every_mode) {
  PointCloud cloud;
  cloud.useIntensity();
  cloud.useColor();
  cloud.useNormal();
  cloud.useCovariance();
  cloud.setFrameId("lidar");
  cloud.setTimestamp(123456789ull);
  for (int i = 0; i < 40; ++i) {
    cloud.add(0.05f * float(i % 10), 0.3f * float(i / 10), 0.01f * float(i));
    cloud.intensity(size_t(i)) = float(i);
    cloud.setColor(size_t(i), Color(uint8_t(i), uint8_t(2 * i), uint8_t(3 * i)));
    cloud.normals()[size_t(i)] = Normal4(0.0f, 0.0f, 1.0f, 0.0f);
  }
  for (auto mode : {filters::VoxelMode::CENTROID, filters::VoxelMode::NEAREST, filters::VoxelMode::ANY, filters::VoxelMode::CENTER}) {
    auto out = filters::voxelGrid(cloud, 0.25f, mode);
    EXPECT_EQ(out.size(), 8u);
    EXPECT_TRUE(out.hasIntensity() && out.hasColor() && out.hasNormal() && out.hasCovariance());
    EXPECT_EQ(out.frameId(), std::string("lidar"));
    EXPECT_EQ(out.timestamp(), 123456789ull);
    for (size_t i = 0; i < out.size(); ++i) EXPECT_EQ(out.normal(i).z(), 1.0f);
  }
  auto center = filters::voxelGrid(cloud, 0.25f, filters::VoxelMode::CENTER);
  EXPECT_EQ(center.point(0).x(), 0.125f);
  EXPECT_EQ(center.point(0).y(), 0.125f);
  auto top = filters::gridMaxZ(cloud, 0.25f);
  ASSERT_EQ(top.size(), 8u);
  EXPECT_EQ(top.intensity(0), 4.0f);  // cell (0, 0): points 0 .. 4, the highest is the last
  EXPECT_EQ(top.color(0).g, 8);
  EXPECT_EQ(top.frameId(), std::string("lidar"));
  EXPECT_EQ(cloud.size(), 40u);
}

TEST(Mirror, sizes_outside_the_range_throw) {
  PointCloud cloud;
  cloud.add(1.0f, 2.0f, 3.0f);
  for (float bad : {0.0009f, 100.5f, 0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN()}) {
    EXPECT_THROW(filters::voxelGrid(cloud, bad), std::invalid_argument);
    EXPECT_THROW(filters::gridMaxZ(cloud, bad), std::invalid_argument);
    EXPECT_THROW(filters::voxelGrid(PointCloud(), bad), std::invalid_argument);
  }
  try {
    filters::voxelGrid(cloud, 101.0f);
  } catch (const std::invalid_argument& e) {
    EXPECT_EQ(std::string(e.what()), std::string("voxel_size must be in [0.001, 100]"));
  }
  try {
    filters::gridMaxZ(cloud, 101.0f);
  } catch (const std::invalid_argument& e) {
    EXPECT_EQ(std::string(e.what()), std::string("grid_size must be in [0.001, 100]"));
  }
  EXPECT_EQ(filters::voxelGrid(cloud, 0.001f).size(), 1u);
  EXPECT_EQ(filters::gridMaxZ(cloud, 100.0f).size(), 1u);
}

TEST(Mirror, the_order_setting_decides_ties) {
  // 40 points of one cell, equally high: gridMaxZ keeps the first of the run — the first point in input order, another
  // one in the order std::sort leaves 40 equal keys in
  PointCloud cloud;
  cloud.useIntensity();
  for (int i = 0; i < 40; ++i) {
    cloud.add(0.1f, 0.1f, 1.0f);
    cloud.intensity(size_t(i)) = float(i);
  }
  EXPECT_EQ(filters::downsampleOrder(), 0);
  auto stable = filters::gridMaxZ(cloud, 1.0f);
  ASSERT_EQ(stable.size(), 1u);
  EXPECT_EQ(stable.intensity(0), 0.0f);
  filters::setDownsampleOrder(1);
  auto sorted = filters::gridMaxZ(cloud, 1.0f);
  filters::setDownsampleOrder(0);
  ASSERT_EQ(sorted.size(), 1u);
  EXPECT_TRUE(sorted.intensity(0) != 0.0f);
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
