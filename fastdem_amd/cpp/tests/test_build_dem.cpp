// test_build_dem — fastdem/io/build_dem.hpp through the C++ host mirror: the BuildDEMTest group of the reference's
// fastdem/tests/test_rasterization.cpp and the statisticalOutlierRemoval tests of nanoPCL's tests/test_filters.cpp, in
// this repository's own words.  Needs the GPU: tests/test_build_dem_cpp_gpu.py.
#include <cmath>

#include "fastdem/io/build_dem.hpp"
#include "mini_test.hpp"

using namespace fastdem;
using nanogrid::Position;
namespace filters = nanopcl::filters;

namespace {
// a square of points `step` apart at height z, without those `skip` names
template <typename Skip>
PointCloud plane(float half, float step, float z, Skip skip) {
  PointCloud c;
  for (float x = -half; x <= half; x += step)
    for (float y = -half; y <= half; y += step)
      if (!skip(x, y)) c.add(x, y, z);
  return c;
}
PointCloud plane(float half, float step, float z) {
  return plane(half, step, z, [](float, float) { return false; });
}
// a 5 x 5 lattice at z = 0 and one point far away
PointCloud latticeWithOutlier(int side) {
  PointCloud c;
  for (int x = 0; x < side; ++x)
    for (int y = 0; y < side; ++y) c.add(float(x), float(y), 0.0f);
  c.add(100.0f, 100.0f, 0.0f);
  return c;
}
}  // namespace

TEST(StatisticalOutlierRemoval, ARegularLatticeKeepsEveryPointUnderAWideThreshold) {
  PointCloud c;
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < 3; ++y)
      for (int z = 0; z < 3; ++z) c.add(float(x), float(y), float(z));
  EXPECT_EQ(filters::statisticalOutlierRemoval(c, 4, 3.0f).size(), size_t(27));
}

TEST(StatisticalOutlierRemoval, TheFarPointGoes) {
  const PointCloud c = latticeWithOutlier(5);
  EXPECT_EQ(c.size(), size_t(26));
  const auto kept = filters::statisticalOutlierRemoval(c, 4, 1.0f);
  EXPECT_TRUE(kept.size() < 26);
  EXPECT_TRUE(kept.size() >= 24);
  for (size_t i = 0; i < kept.size(); ++i) EXPECT_TRUE(kept.point(i)[0] < 50.0f);
}

TEST(StatisticalOutlierRemoval, ChannelsFrameAndStampSurvive) {
  PointCloud c;
  c.useIntensity();
  c.useColor();
  for (int i = 0; i < 9; ++i) {
    c.add(float(i % 3), float(i / 3), 0.0f, nanopcl::Intensity(float(i) * 0.1f));
    c.setColor(size_t(i), Color(uint8_t(i * 10), uint8_t(i * 20), uint8_t(i * 30)));
  }
  c.add(100.0f, 100.0f, 0.0f, nanopcl::Intensity(0.99f));
  c.setColor(9, Color(255, 255, 255));
  c.setFrameId("map");
  c.setTimestamp(42);
  const auto kept = filters::statisticalOutlierRemoval(c, 3, 1.0f);
  EXPECT_TRUE(kept.hasIntensity());
  EXPECT_TRUE(kept.hasColor());
  EXPECT_EQ(kept.size(), size_t(9));
  EXPECT_TRUE(kept.color(0).r < 200);
  EXPECT_FLOAT_EQ(kept.intensity(4), 0.4f);
  EXPECT_EQ(int(kept.color(8).g), 160);
  EXPECT_TRUE(kept.frameId() == "map");
  EXPECT_EQ(kept.timestamp(), uint64_t(42));
}

TEST(StatisticalOutlierRemoval, NoNeighboursNoPoints) {
  EXPECT_TRUE(filters::statisticalOutlierRemoval(PointCloud{}, 10).empty());
  EXPECT_TRUE(filters::statisticalOutlierRemoval(latticeWithOutlier(5), 0).empty());
  PointCloud one;
  one.add(1.0f, 2.0f, 3.0f);
  EXPECT_TRUE(filters::statisticalOutlierRemoval(one, 10).empty());
  EXPECT_TRUE(filters::statisticalOutlierRemoval(latticeWithOutlier(5), 4, 1.0f).size() >= 24);
}

TEST(BuildDEM, AnEmptyCloudGivesAMapWithoutGeometry) {
  EXPECT_FALSE(buildDEM(PointCloud{}).isInitialized());
}

TEST(BuildDEM, AGroundPlaneComesThrough) {
  DEMConfig config;
  config.resolution = 0.5f;
  config.sor_k = 5;
  config.inpaint_iterations = 0;
  auto map = buildDEM(plane(2.0f, 0.1f, 0.0f), config);
  EXPECT_TRUE(map.isInitialized());
  EXPECT_TRUE(map.exists(layer::elevation));
  EXPECT_TRUE(map.hasElevationAt(Position(0.0, 0.0)));
  EXPECT_NEAR(map.elevationAt(Position(0.0, 0.0)), 0.0f, 0.1f);
}

TEST(BuildDEM, InpaintingClosesAGap) {
  DEMConfig config;
  config.resolution = 0.5f;
  config.sor_k = 5;
  config.inpaint_iterations = 3;
  const auto gap = [](float x, float y) { return std::abs(x) < 0.3f && std::abs(y) < 0.3f; };
  auto filled = buildDEM(plane(2.0f, 0.1f, 1.0f, gap), config);
  EXPECT_TRUE(filled.isInitialized());
  EXPECT_TRUE(filled.hasElevationAt(Position(0.0, 0.0)));
  EXPECT_NEAR(filled.elevationAt(Position(0.0, 0.0)), 1.0f, 1e-3f);
}

TEST(BuildDEM, TheResolutionIsTheConfigs) {
  PointCloud c;
  c.add(0.0f, 0.0f, 1.0f);
  c.add(1.0f, 1.0f, 2.0f);
  DEMConfig config;
  config.resolution = 0.25f;
  config.sor_k = 1;
  config.inpaint_iterations = 0;
  EXPECT_FLOAT_EQ(float(buildDEM(c, config).getResolution()), 0.25f);
}

TEST(BuildDEM, TheStatisticsLayersExist) {
  DEMConfig config;
  config.resolution = 0.5f;
  config.sor_k = 3;
  config.inpaint_iterations = 0;
  auto map = buildDEM(plane(1.0f, 0.2f, 0.5f), config);
  EXPECT_TRUE(map.exists(layer::elevation));
  EXPECT_TRUE(map.exists(layer::elevation_min));
  EXPECT_TRUE(map.exists(layer::elevation_max));
  EXPECT_TRUE(map.exists(layer::variance));
  EXPECT_TRUE(map.exists(layer::n_points));
}

TEST(BuildDEM, ACloudTheOutlierRemovalEmptiesGivesNoMap) {
  PointCloud one;
  one.add(1.0f, 2.0f, 3.0f);
  EXPECT_FALSE(buildDEM(one).isInitialized());
  DEMConfig config;
  config.sor_k = 0;
  EXPECT_FALSE(buildDEM(plane(1.0f, 0.2f, 0.5f), config).isInitialized());
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
