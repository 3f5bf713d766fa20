// test_pcd_convert — fastdem/io/pcd_convert.hpp through the C++ host mirror: the FromPointCloudTest,
// FromPointCloudStatsTest and ToPointCloudTest groups of the reference's fastdem/tests/test_rasterization.cpp, in this
// repository's own words (its BuildDEMTest group is out of scope).  Needs the GPU: tests/test_pcd_convert_cpp_gpu.py.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fastdem/io/pcd_convert.hpp"
#include "mini_test.hpp"

using namespace fastdem;
using nanogrid::Index;
using nanogrid::Position;

namespace {
ElevationMap makeMap() { return ElevationMap(10.0f, 10.0f, 0.5f, "map"); }  // 20 x 20 cells around the origin
// three points that share the cell of (0.1, 0.1)
PointCloud oneCell(float z0, float z1, float z2) {
  PointCloud c;
  c.add(0.1f, 0.1f, z0);
  c.add(0.15f, 0.15f, z1);
  c.add(0.2f, 0.2f, z2);
  return c;
}
size_t finiteCells(const ElevationMap& m, const char* l) {
  const auto& d = m.get(l);
  size_t n = 0;
  for (size_t k = 0; k < d.size(); ++k) n += std::isfinite(d.data()[k]) ? 1 : 0;
  return n;
}
}  // namespace

TEST(FromPointCloud, AnEmptyCloudLeavesTheMapAlone) {
  auto map = makeMap();
  const auto before = map.getLayers();
  fromPointCloud(PointCloud{}, map);
  EXPECT_TRUE(map.isEmpty());
  EXPECT_TRUE(map.getLayers() == before);
}

TEST(FromPointCloud, ACloudOutsideTheMapCreatesNoLayer) {
  auto map = makeMap();
  PointCloud c;
  c.add(50.0f, 50.0f, 1.0f);
  fromPointCloud(c, map);
  EXPECT_TRUE(map.isEmpty());
  EXPECT_FALSE(map.exists(layer::variance));
}

TEST(FromPointCloud, ElevationLandsInThePointsCells) {
  auto map = makeMap();
  PointCloud c;
  c.add(1.0f, 1.0f, 2.5f);
  c.add(-2.0f, 3.0f, -0.5f);
  fromPointCloud(c, map);
  EXPECT_FLOAT_EQ(map.elevationAt(Position(1.0, 1.0)), 2.5f);
  EXPECT_FLOAT_EQ(map.elevationAt(Position(-2.0, 3.0)), -0.5f);
  EXPECT_EQ(finiteCells(map, layer::elevation), size_t(2));
}

TEST(FromPointCloud, MaxMinMeanPickWithinACell) {
  auto a = makeMap(), b = makeMap(), c = makeMap(), d = makeMap();
  fromPointCloud(oneCell(1.0f, 5.0f, 3.0f), a, RasterMethod::Max);
  fromPointCloud(oneCell(1.0f, 5.0f, 3.0f), b, RasterMethod::Min);
  fromPointCloud(oneCell(1.0f, 5.0f, 3.0f), c, RasterMethod::Mean);
  fromPointCloud(oneCell(1.0f, 5.0f, 3.0f), d, RasterMethod::MinMax);
  EXPECT_FLOAT_EQ(a.elevationAt(Position(0.1, 0.1)), 5.0f);
  EXPECT_FLOAT_EQ(b.elevationAt(Position(0.1, 0.1)), 1.0f);
  EXPECT_FLOAT_EQ(c.elevationAt(Position(0.1, 0.1)), 3.0f);
  EXPECT_FLOAT_EQ(d.elevationAt(Position(0.1, 0.1)), 5.0f);
  EXPECT_FLOAT_EQ(d.atPosition(layer::elevation_min, Position(0.1, 0.1)), 1.0f);
}

TEST(FromPointCloud, IntensityGoesIntoAnExistingLayer) {
  auto map = makeMap();
  map.add(layer::intensity);
  PointCloud c;
  c.add(0.1f, 0.1f, 1.0f, nanopcl::Intensity(0.7f));
  fromPointCloud(c, map);
  EXPECT_FLOAT_EQ(map.atPosition(layer::intensity, Position(0.1, 0.1)), 0.7f);
}

TEST(FromPointCloud, ColourIsPackedIntoItsLayer) {
  auto map = makeMap();
  map.add(layer::color);
  PointCloud c;
  c.add(0.1f, 0.1f, 1.0f, Color(255, 128, 64));
  fromPointCloud(c, map);
  const float packed = map.atPosition(layer::color, Position(0.1, 0.1));
  uint32_t bits = 0;
  std::memcpy(&bits, &packed, sizeof(bits));
  EXPECT_EQ(bits, 0x00FF8040u);
}

TEST(FromPointCloud, AnAutoSizedMapHoldsEveryPoint) {
  PointCloud c;
  c.add(-5.0f, -3.0f, 1.0f);
  c.add(5.0f, 3.0f, 2.0f);
  c.add(0.0f, 0.0f, 1.5f);
  auto map = fromPointCloud(c, 0.5f);
  ASSERT_TRUE(map.isInitialized());
  for (const Position& p : {Position(-5.0, -3.0), Position(5.0, 3.0), Position(0.0, 0.0)}) {
    EXPECT_TRUE(map.isInside(p));
    EXPECT_TRUE(map.hasElevationAt(p));
  }
  EXPECT_NEAR(map.getLength()(0), 10.5, 0.5);
  EXPECT_NEAR(map.getLength()(1), 6.5, 0.5);
  EXPECT_FLOAT_EQ(map.getResolution(), 0.5f);
  EXPECT_TRUE(map.exists(layer::variance) && map.exists(layer::n_points));
}

TEST(FromPointCloud, AnAutoSizedMapOfNothingHasNoGeometry) {
  auto map = fromPointCloud(PointCloud{}, 0.5f);
  EXPECT_FALSE(map.isInitialized());
}

TEST(FromPointCloudStats, TheStatisticsLayersAppear) {
  auto map = makeMap();
  PointCloud c;
  c.add(0.1f, 0.1f, 1.0f);
  fromPointCloud(c, map);
  for (const char* l : {layer::elevation_min, layer::elevation_max, layer::variance, layer::n_points})
    EXPECT_TRUE(map.exists(l));
  EXPECT_FALSE(map.exists(layer::intensity));
}

TEST(FromPointCloudStats, MinMaxAndCount) {
  auto map = makeMap();
  fromPointCloud(oneCell(1.0f, 5.0f, 3.0f), map);
  const Position p(0.1, 0.1);
  EXPECT_FLOAT_EQ(map.atPosition(layer::elevation_min, p), 1.0f);
  EXPECT_FLOAT_EQ(map.atPosition(layer::elevation_max, p), 5.0f);
  EXPECT_FLOAT_EQ(map.atPosition(layer::n_points, p), 3.0f);
}

TEST(FromPointCloudStats, VarianceIsTheSampleVariance) {
  auto map = makeMap();
  fromPointCloud(oneCell(2.0f, 4.0f, 6.0f), map, RasterMethod::Mean);   // mean 4, sum of squares 8, / 2
  const Position p(0.1, 0.1);
  EXPECT_FLOAT_EQ(map.elevationAt(p), 4.0f);
  EXPECT_FLOAT_EQ(map.atPosition(layer::variance, p), 4.0f);
}

TEST(FromPointCloudStats, OnePointHasNoVariance) {
  auto map = makeMap();
  PointCloud c;
  c.add(1.0f, 1.0f, 7.0f);
  fromPointCloud(c, map);
  EXPECT_FLOAT_EQ(map.atPosition(layer::variance, Position(1.0, 1.0)), 0.0f);
  EXPECT_FLOAT_EQ(map.atPosition(layer::n_points, Position(1.0, 1.0)), 1.0f);
}

TEST(FromPointCloudStats, TheIntensityLayerIsCreatedOnDemand) {
  auto map = makeMap();
  PointCloud c;
  c.add(0.1f, 0.1f, 1.0f, nanopcl::Intensity(0.7f));
  fromPointCloud(c, map);
  ASSERT_TRUE(map.exists(layer::intensity));
  EXPECT_FLOAT_EQ(map.atPosition(layer::intensity, Position(0.1, 0.1)), 0.7f);
}

TEST(FromPointCloudStats, NaNHeightsDoNotCount) {
  auto map = makeMap();
  fromPointCloud(oneCell(NAN, 2.0f, 4.0f), map);
  const Position p(0.1, 0.1);
  EXPECT_FLOAT_EQ(map.atPosition(layer::n_points, p), 2.0f);
  EXPECT_FLOAT_EQ(map.atPosition(layer::elevation_max, p), 4.0f);
  EXPECT_FLOAT_EQ(map.atPosition(layer::elevation_min, p), 2.0f);
}

TEST(ToPointCloud, AnEmptyMapIsAnEmptyCloud) {
  auto map = makeMap();
  EXPECT_TRUE(toPointCloud(map).empty());
}

TEST(ToPointCloud, ValidCellsBecomePointsAtTheirCentres) {
  auto map = makeMap();
  map.at(layer::elevation, Index(3, 4)) = 1.5f;
  map.at(layer::elevation, Index(10, 12)) = -2.0f;
  const auto cloud = toPointCloud(map);
  ASSERT_EQ(cloud.size(), size_t(2));
  std::vector<float> zs = {cloud.point(0).z(), cloud.point(1).z()};
  std::sort(zs.begin(), zs.end());
  EXPECT_FLOAT_EQ(zs[0], -2.0f);
  EXPECT_FLOAT_EQ(zs[1], 1.5f);
  for (size_t i = 0; i < cloud.size(); ++i) {
    Index idx;
    ASSERT_TRUE(map.getIndex(Position(cloud.point(i).x(), cloud.point(i).y()), idx));
    Position centre;
    ASSERT_TRUE(map.getPosition(idx, centre));
    EXPECT_NEAR(centre(0), cloud.point(i).x(), 1e-5);
    EXPECT_NEAR(centre(1), cloud.point(i).y(), 1e-5);
    EXPECT_FLOAT_EQ(map.elevationAt(idx), cloud.point(i).z());
  }
  EXPECT_FALSE(cloud.hasIntensity());
  EXPECT_FALSE(cloud.hasColor());
}

TEST(ToPointCloud, IntensityAndColourSurvive) {
  auto map = makeMap();
  PointCloud c;
  c.useIntensity();
  c.add(0.1f, 0.1f, 1.0f, Color(10, 20, 30));
  c.intensity(0) = 0.25f;
  fromPointCloud(c, map);
  const auto out = toPointCloud(map);
  ASSERT_EQ(out.size(), size_t(1));
  ASSERT_TRUE(out.hasIntensity() && out.hasColor());
  EXPECT_FLOAT_EQ(out.intensity(0), 0.25f);
  EXPECT_EQ(int(out.color(0).r), 10);
  EXPECT_EQ(int(out.color(0).g), 20);
  EXPECT_EQ(int(out.color(0).b), 30);
}

TEST(ToPointCloud, ARoundTripKeepsTheCellCount) {
  PointCloud c;
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 6; ++j) c.add(-3.0f + float(i), -2.0f + float(j), 0.1f * float(i + j));
  auto map = makeMap();
  fromPointCloud(c, map);
  const auto out = toPointCloud(map);
  EXPECT_EQ(out.size(), finiteCells(map, layer::elevation));
  EXPECT_EQ(out.size(), size_t(48));
  auto again = makeMap();
  fromPointCloud(out, again);
  EXPECT_EQ(finiteCells(again, layer::elevation), size_t(48));
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
