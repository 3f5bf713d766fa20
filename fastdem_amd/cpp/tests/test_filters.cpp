// test_filters.cpp — the filter cases of nanoPCL's tests (lib/nanoPCL/tests/test_filters.cpp: removeInvalid :99-110, the
// crop group :118-153, the four radiusOutlierRemoval tests :323-384 and the radius parts of its two boundary tests
// :460-480) at their own bounds, re-expressed on the mirror's nanopcl/filters/{core,crop,outlier_removal}.hpp.  Plus what
// the mirror states beyond the reference: the const& and && overloads agree, every channel and the metadata are kept,
// the refusals.  Needs a device (tests/test_filters_cpp_gpu.py runs it).
#include <cmath>
#include <limits>
#include <stdexcept>
#include <utility>

#include "mini_test.hpp"
#include "nanopcl/filters/crop.hpp"
#include "nanopcl/filters/outlier_removal.hpp"

using nanopcl::Color;
using nanopcl::Intensity;
using nanopcl::Point;
using nanopcl::PointCloud;
namespace filters = nanopcl::filters;

namespace {
PointCloud grid3x3x3() {  // 27 points
  PointCloud cloud;
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < 3; ++y)
      for (int z = 0; z < 3; ++z) cloud.add(float(x), float(y), float(z));
  return cloud;
}
PointCloud lineWithOutlier(int n) {  // n points 0.1 apart and one 100 away
  PointCloud cloud;
  for (int i = 0; i < n; ++i) cloud.add(float(i) * 0.1f, 0.0f, 0.0f);
  cloud.add(100.0f, 0.0f, 0.0f);
  return cloud;
}
bool same(const PointCloud& a, const PointCloud& b) {
  if (a.size() != b.size() || a.frameId() != b.frameId() || a.timestamp() != b.timestamp()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a.xData()[i] != b.xData()[i] || a.yData()[i] != b.yData()[i] || a.zData()[i] != b.zData()[i]) return false;
  return true;
}
}  // namespace

// ---- core and crops (:99-153) ----
TEST(Filters, removeInvalid) {
  PointCloud cloud;
  cloud.add(1.0f, 2.0f, 3.0f);
  cloud.add(std::numeric_limits<float>::quiet_NaN(), 0, 0);
  cloud.add(0, std::numeric_limits<float>::infinity(), 0);
  cloud.add(4.0f, 5.0f, 6.0f);
  ASSERT_EQ(cloud.size(), 4u);
  const auto cleaned = filters::removeInvalid(cloud);
  ASSERT_EQ(cleaned.size(), 2u);
  EXPECT_NEAR(cleaned.point(0).x(), 1.0f, 0.01f);
  EXPECT_NEAR(cleaned.point(1).x(), 4.0f, 0.01f);
}

TEST(Filters, cropBox_inside) {
  const PointCloud cloud = grid3x3x3();
  const auto cropped = filters::cropBox(cloud, Point(0.5f, 0.5f, 0.5f), Point(1.5f, 1.5f, 1.5f), filters::FilterMode::INSIDE);
  ASSERT_EQ(cropped.size(), 1u);  // only (1, 1, 1)
  EXPECT_NEAR(cropped.point(0).x(), 1.0f, 0.01f);
}

TEST(Filters, cropBox_outside) {
  const PointCloud cloud = grid3x3x3();
  const auto cropped = filters::cropBox(cloud, Point(0.5f, 0.5f, 0.5f), Point(1.5f, 1.5f, 1.5f), filters::FilterMode::OUTSIDE);
  ASSERT_EQ(cropped.size(), 26u);
}

TEST(Filters, cropRange) {
  PointCloud cloud;
  cloud.add(0, 0, 0);
  cloud.add(1, 0, 0);
  cloud.add(2, 0, 0);
  cloud.add(10, 0, 0);
  const auto cropped = filters::cropRange(cloud, 0.5f, 5.0f);
  ASSERT_EQ(cropped.size(), 2u);  // the distances 1 and 2
}

TEST(Filters, cropZ) {
  const PointCloud cloud = grid3x3x3();
  const auto cropped = filters::cropZ(cloud, 1.0f, 1.0f);
  ASSERT_EQ(cropped.size(), 9u);  // 3 x 3 points at z = 1
}

// ---- radius outlier removal (:323-384, :460-480) ----
TEST(Filters, radiusOutlierRemoval_basic) {
  const PointCloud cloud = lineWithOutlier(10);
  ASSERT_EQ(cloud.size(), 11u);
  const auto filtered = filters::radiusOutlierRemoval(cloud, 0.5f, 2);
  ASSERT_EQ(filtered.size(), 10u);  // the isolated point has no neighbour within the radius
}

TEST(Filters, radiusOutlierRemoval_all_inliers) {
  PointCloud cloud;
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < 3; ++y) cloud.add(float(x) * 0.5f, float(y) * 0.5f, 0.0f);
  const auto filtered = filters::radiusOutlierRemoval(cloud, 1.0f, 1);
  ASSERT_EQ(filtered.size(), 9u);
}

TEST(Filters, radiusOutlierRemoval_channel_preservation) {
  PointCloud cloud;
  cloud.useIntensity();
  for (int i = 0; i < 5; ++i) cloud.add(float(i) * 0.1f, 0.0f, 0.0f, Intensity(float(i) * 0.2f));
  cloud.add(100.0f, 0.0f, 0.0f, Intensity(0.99f));
  const auto filtered = filters::radiusOutlierRemoval(cloud, 0.5f, 2);
  ASSERT_TRUE(filtered.hasIntensity());
  ASSERT_EQ(filtered.size(), 5u);
  EXPECT_NEAR(filtered.intensity(0), 0.0f, 0.01f);
  EXPECT_NEAR(filtered.intensity(4), 0.8f, 0.01f);
}

TEST(Filters, radiusOutlierRemoval_move) {
  PointCloud cloud = lineWithOutlier(10);
  const auto filtered = filters::radiusOutlierRemoval(std::move(cloud), 0.5f, 2);
  ASSERT_EQ(filtered.size(), 10u);
}

TEST(Filters, outlierRemoval_empty_cloud) {
  const PointCloud empty;
  const auto radius_filtered = filters::radiusOutlierRemoval(empty, 1.0f, 3);
  ASSERT_TRUE(radius_filtered.empty());
}

TEST(Filters, outlierRemoval_single_point) {
  PointCloud single;
  single.add(1.0f, 2.0f, 3.0f);
  const auto radius_filtered = filters::radiusOutlierRemoval(single, 1.0f, 1);  // a single point has no neighbour
  ASSERT_TRUE(radius_filtered.empty());
  EXPECT_EQ(filters::radiusOutlierRemoval(single, 1.0f, 0).size(), 1u);
}

// ---- what the mirror states beyond the reference ----
TEST(Mirror, overloads_agree) {
  const PointCloud cloud = grid3x3x3();
  const Point lo(0.5f, -1.0f, 0.0f), hi(2.0f, 1.0f, 1.5f);
  for (const auto mode : {filters::FilterMode::INSIDE, filters::FilterMode::OUTSIDE}) {
    EXPECT_TRUE(same(filters::cropBox(cloud, lo, hi, mode), filters::cropBox(PointCloud(cloud), lo, hi, mode)));
    EXPECT_TRUE(same(filters::cropRange(cloud, 1.0f, 2.5f, mode), filters::cropRange(PointCloud(cloud), 1.0f, 2.5f, mode)));
    EXPECT_TRUE(same(filters::cropX(cloud, 1.0f, 2.0f, mode), filters::cropX(PointCloud(cloud), 1.0f, 2.0f, mode)));
    EXPECT_TRUE(same(filters::cropY(cloud, 0.0f, 0.5f, mode), filters::cropY(PointCloud(cloud), 0.0f, 0.5f, mode)));
    EXPECT_TRUE(same(filters::cropZ(cloud, 2.0f, 1.0f, mode), filters::cropZ(PointCloud(cloud), 2.0f, 1.0f, mode)));
    EXPECT_TRUE(same(filters::cropAngle(cloud, 0.1f, 1.0f, mode), filters::cropAngle(PointCloud(cloud), 0.1f, 1.0f, mode)));
    // the two modes of a crop without a NaN split the cloud
    EXPECT_EQ(filters::cropBox(cloud, lo, hi, filters::FilterMode::INSIDE).size() +
                  filters::cropBox(cloud, lo, hi, filters::FilterMode::OUTSIDE).size(), cloud.size());
  }
  EXPECT_EQ(filters::cropX(cloud, 1.0f, 2.0f).size(), 18u);
  EXPECT_EQ(filters::cropZ(cloud, 2.0f, 1.0f).size(), 0u);  // min > max: not refused, nothing inside
  EXPECT_EQ(filters::cropZ(cloud, 2.0f, 1.0f, filters::FilterMode::OUTSIDE).size(), 27u);
  EXPECT_TRUE(same(filters::removeInvalid(cloud), filters::removeInvalid(PointCloud(cloud))));
  EXPECT_TRUE(same(filters::radiusOutlierRemoval(cloud, 1.0f, 4), filters::radiusOutlierRemoval(PointCloud(cloud), 1.0f, 4)));
  EXPECT_EQ(filters::radiusOutlierRemoval(cloud, 1.0f, 4).size(), 19u);  // all but the 8 corners, which have 3
  const auto even = filters::filter(cloud, [](size_t i) { return i % 2 == 0; });
  EXPECT_EQ(even.size(), 14u);
  EXPECT_TRUE(same(even, filters::filter(PointCloud(cloud), [](size_t i) { return i % 2 == 0; })));
}

TEST(Mirror, channels_and_metadata_kept) {
  PointCloud cloud;
  cloud.useIntensity();
  cloud.useColor();
  cloud.useNormal();
  cloud.useCovariance();
  cloud.useLabel();
  for (int i = 0; i < 10; ++i) {
    cloud.add(float(i) * 0.1f, 0.0f, 0.0f, Intensity(float(i) * 0.1f));
    cloud.setColor(size_t(i), Color(uint8_t(i * 10), uint8_t(i * 20), uint8_t(i)));
    cloud.normal(size_t(i)) = nanopcl::Normal4(0.0f, float(i), 1.0f, 0.0f);
    cloud.covarianceData()[i * 9] = float(i);
    cloud.label(size_t(i)) = nanopcl::Label(uint32_t(i) + 7u);
  }
  cloud.add(100.0f, 0.0f, 0.0f, Intensity(0.99f));
  cloud.setFrameId("lidar");
  cloud.setTimestamp(123456789u);
  const auto check = [&](const PointCloud& out, size_t first, size_t count) {
    ASSERT_EQ(out.size(), count);
    ASSERT_TRUE(out.hasIntensity() && out.hasColor() && out.hasNormal() && out.hasCovariance() && out.hasLabel());
    EXPECT_TRUE(out.frameId() == "lidar");
    EXPECT_EQ(out.timestamp(), 123456789u);
    for (size_t k = 0; k < count; ++k) {
      const size_t i = first + k;
      EXPECT_FLOAT_EQ(out.point(k).x(), float(i) * 0.1f);
      EXPECT_FLOAT_EQ(out.intensity(k), float(i) * 0.1f);
      EXPECT_EQ(int(out.color(k).g), int(i * 20));
      EXPECT_FLOAT_EQ(out.normal(k).y(), float(i));
      EXPECT_FLOAT_EQ(out.covariance(k)(0, 0), float(i));
      EXPECT_EQ(out.label(k).val, uint32_t(i) + 7u);
    }
  };
  check(filters::radiusOutlierRemoval(cloud, 0.5f, 2), 0, 10);
  check(filters::cropX(cloud, 0.25f, 0.65f), 3, 4);
  check(filters::cropRange(PointCloud(cloud), 0.0f, 50.0f), 0, 10);
  const auto all = filters::removeInvalid(cloud);  // no invalid point: every point stays
  ASSERT_EQ(all.size(), 11u);
  EXPECT_TRUE(all.frameId() == "lidar" && all.hasLabel());
  EXPECT_FLOAT_EQ(all.intensity(10), 0.99f);
}

TEST(Mirror, refusals) {
  PointCloud cloud = lineWithOutlier(10);
  EXPECT_THROW((void)filters::radiusOutlierRemoval(cloud, 0.0f, 2), std::runtime_error);
  EXPECT_THROW((void)filters::radiusOutlierRemoval(cloud, -1.0f, 2), std::runtime_error);
  EXPECT_THROW((void)filters::radiusOutlierRemoval(cloud, std::numeric_limits<float>::quiet_NaN(), 2), std::runtime_error);
  EXPECT_THROW((void)filters::radiusOutlierRemoval(cloud, std::numeric_limits<float>::infinity(), 2), std::runtime_error);
  EXPECT_THROW((void)filters::radiusOutlierRemoval(cloud, 1e-5f, 2), std::runtime_error);  // 100 m is beyond 2^20 voxels
  cloud.point(3) = Eigen::Vector3f(std::numeric_limits<float>::quiet_NaN(), 0.0f, 0.0f);
  EXPECT_THROW((void)filters::radiusOutlierRemoval(cloud, 0.5f, 2), std::runtime_error);
  EXPECT_EQ(filters::radiusOutlierRemoval(filters::removeInvalid(cloud), 0.5f, 2).size(), 9u);  // what the user calls first
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
