// test_pcd_io.cpp — nanoPCL's six PCD tests (lib/nanoPCL/tests/test_io.cpp: pcd_ascii_roundtrip, pcd_binary_roundtrip,
// pcd_viewpoint, pcd_rgb_channel, pcd_empty_cloud, pcd_exception_on_bad_stream) re-expressed on the mirror's
// nanopcl/io/pcd_io.hpp, and one round trip in the shape of the pcd2dem tool.  Needs a device: binary records are decoded
// and packed there (tests/test_pcd_io_cpp_gpu.py runs it).
#include <cstdio>
#include <fstream>
#include <sstream>

#include "fastdem/io/build_dem.hpp"
#include "mini_test.hpp"
#include "nanopcl/io/pcd_io.hpp"

using nanopcl::Color;
using nanopcl::Intensity;
using nanopcl::Normal4;
using nanopcl::PointCloud;
namespace io = nanopcl::io;

constexpr float EPS = 1e-5f;

TEST(PcdIO, pcd_ascii_roundtrip) {
  PointCloud cloud;
  cloud.useIntensity();
  cloud.add(1.0f, 2.0f, 3.0f, Intensity(100.0f));
  cloud.add(4.0f, 5.0f, 6.0f, Intensity(200.0f));
  std::stringstream ss;
  io::PCDSaveOptions opts;
  opts.format = io::PCDFormat::ASCII;
  io::savePCD(ss, cloud, opts);
  ss.seekg(0);
  io::PCDMetadata metadata;
  PointCloud loaded = io::loadPCD(ss, metadata);
  ASSERT_EQ(loaded.size(), 2u);
  EXPECT_NEAR(loaded.point(0).x(), 1.0f, EPS);
  EXPECT_NEAR(loaded.point(0).y(), 2.0f, EPS);
  EXPECT_NEAR(loaded.point(0).z(), 3.0f, EPS);
  EXPECT_NEAR(loaded.point(1).x(), 4.0f, EPS);
  ASSERT_TRUE(loaded.hasIntensity());
  EXPECT_NEAR(loaded.intensity(0), 100.0f, EPS);
  EXPECT_NEAR(loaded.intensity(1), 200.0f, EPS);
  EXPECT_FALSE(loaded.hasColor());
  EXPECT_FALSE(loaded.hasNormal());
}

TEST(PcdIO, pcd_binary_roundtrip) {
  PointCloud cloud;
  cloud.useIntensity();
  cloud.useNormal();
  cloud.add(1.5f, 2.5f, 3.5f);
  cloud.intensity(cloud.size() - 1) = 50.0f;
  cloud.normals().back() = Normal4(0.0f, 0.0f, 1.0f, 0.0f);
  cloud.add(-1.0f, -2.0f, -3.0f);
  cloud.intensity(cloud.size() - 1) = 75.0f;
  cloud.normals().back() = Normal4(1.0f, 0.0f, 0.0f, 0.0f);
  std::stringstream ss(std::ios::binary | std::ios::in | std::ios::out);
  io::PCDSaveOptions opts;
  opts.format = io::PCDFormat::BINARY;
  io::savePCD(ss, cloud, opts);
  ss.seekg(0);
  io::PCDMetadata metadata;
  PointCloud loaded = io::loadPCD(ss, metadata);
  ASSERT_EQ(loaded.size(), 2u);
  EXPECT_EQ(metadata.num_points, 2u);
  EXPECT_NEAR(loaded.point(0).x(), 1.5f, EPS);
  EXPECT_NEAR(loaded.point(1).z(), -3.0f, EPS);
  ASSERT_TRUE(loaded.hasIntensity());
  EXPECT_NEAR(loaded.intensity(0), 50.0f, EPS);
  ASSERT_TRUE(loaded.hasNormal());
  EXPECT_NEAR(loaded.normal(0).z(), 1.0f, EPS);
  EXPECT_NEAR(loaded.normal(1).x(), 1.0f, EPS);
  EXPECT_EQ(loaded.normal(1).w(), 0.0f);
}

TEST(PcdIO, pcd_viewpoint) {
  PointCloud cloud;
  cloud.add(0, 0, 0);
  io::PCDSaveOptions opts;
  opts.format = io::PCDFormat::ASCII;
  opts.viewpoint = Eigen::Isometry3d::Identity();
  opts.viewpoint.translation() = Eigen::Vector3d(1.0, 2.0, 3.0);
  opts.viewpoint.rotate(Eigen::AngleAxisd(0.5, Eigen::Vector3d::UnitZ()));
  std::stringstream ss;
  io::savePCD(ss, cloud, opts);
  ss.seekg(0);
  io::PCDMetadata meta;
  io::loadPCD(ss, meta);
  EXPECT_NEAR(meta.viewpoint.translation().x(), 1.0, 1e-9);
  EXPECT_NEAR(meta.viewpoint.translation().y(), 2.0, 1e-9);
  EXPECT_NEAR(meta.viewpoint.translation().z(), 3.0, 1e-9);
  // the rotation through the header's quaternion: its components are printed to six significant digits (at most 5e-7
  // each, under 4e-6 on a matrix entry), so 1e-5 has margin without hiding a wrong formula
  for (int axis = 0; axis < 3; ++axis) {
    Eigen::Isometry3d vp = Eigen::Isometry3d::Identity();
    Eigen::Vector3d ax = axis == 0 ? Eigen::Vector3d::UnitX() : (axis == 1 ? Eigen::Vector3d::UnitY() : Eigen::Vector3d::UnitZ());
    vp.rotate(Eigen::AngleAxisd(0.5, Eigen::Vector3d::UnitZ()));
    vp.rotate(Eigen::AngleAxisd(2.9 - 0.3 * axis, ax));  // a trace below zero: the other branch of the conversion
    opts.viewpoint = vp;
    std::stringstream s2;
    io::savePCD(s2, cloud, opts);
    s2.seekg(0);
    io::loadPCD(s2, meta);
    const Eigen::Matrix3d A = vp.rotation(), B = meta.viewpoint.rotation();
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) EXPECT_NEAR(A(r, c), B(r, c), 1e-5);
  }
}

TEST(PcdIO, pcd_rgb_channel) {
  PointCloud cloud;
  cloud.useColor();
  cloud.add(0, 0, 0);
  cloud.setColor(cloud.size() - 1, Color(255, 128, 64));
  std::stringstream ss;
  io::PCDSaveOptions opts;
  opts.format = io::PCDFormat::BINARY;
  io::savePCD(ss, cloud, opts);
  ss.seekg(0);
  io::PCDMetadata meta;
  PointCloud loaded = io::loadPCD(ss, meta);
  ASSERT_TRUE(loaded.hasColor());
  ASSERT_EQ(loaded.size(), 1u);
  EXPECT_EQ(static_cast<int>(loaded.color(0).r), 255);
  EXPECT_EQ(static_cast<int>(loaded.color(0).g), 128);
  EXPECT_EQ(static_cast<int>(loaded.color(0).b), 64);
}

TEST(PcdIO, pcd_empty_cloud) {
  PointCloud empty;
  std::stringstream ss;
  io::PCDSaveOptions opts;
  opts.format = io::PCDFormat::ASCII;
  io::savePCD(ss, empty, opts);
  ss.seekg(0);
  io::PCDMetadata meta;
  PointCloud loaded = io::loadPCD(ss, meta);
  EXPECT_TRUE(loaded.empty());
  EXPECT_EQ(meta.num_points, 0u);
}

TEST(PcdIO, pcd_exception_on_bad_stream) {
  std::ifstream bad_stream("nonexistent_file_12345.pcd");
  io::PCDMetadata meta;
  EXPECT_THROW(io::loadPCD(bad_stream, meta), io::IOException);
  EXPECT_THROW(io::loadPCD("nonexistent_file_12345.pcd"), io::IOException);
  std::stringstream compressed("FIELDS x y z\nWIDTH 1\nDATA binary_compressed\n");
  EXPECT_THROW(io::loadPCD(compressed, meta), io::IOException);
  std::stringstream short_body("FIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nWIDTH 2\nDATA binary\n0123456789ab");
  EXPECT_THROW(io::loadPCD(short_body, meta), io::IOException);
}

// loadPCD -> buildDEM -> toPointCloud -> savePCD -> loadPCD, through files, as the pcd2dem tool goes
TEST(PcdIO, pcd2dem_roundtrip) {
  PointCloud cloud;
  cloud.useIntensity();
  unsigned s = 12345u;
  auto rnd = [&s] { s = s * 1664525u + 1013904223u; return float(s >> 8) / float(1u << 24); };
  for (int i = 0; i < 900; ++i) {
    const float x = -1.5f + 3.0f * rnd(), y = -1.0f + 2.0f * rnd();
    cloud.add(x, y, 0.2f * x + 0.01f * rnd(), Intensity(rnd()));
  }
  const std::string in = "fdm_test_pcd_io_in.pcd", out = "fdm_test_pcd_io_out.pcd";
  io::savePCD(in, cloud);
  PointCloud loaded = io::loadPCD(in);
  ASSERT_EQ(loaded.size(), cloud.size());
  for (size_t i = 0; i < cloud.size(); i += 97) {
    EXPECT_EQ(loaded.point(i).x(), cloud.point(i).x());
    EXPECT_EQ(loaded.intensity(i), cloud.intensity(i));
  }
  fastdem::DEMConfig config;
  config.resolution = 0.2f;
  auto dem = fastdem::buildDEM(loaded, config);
  ASSERT_TRUE(dem.hasEngine());
  PointCloud cells = fastdem::toPointCloud(dem);
  EXPECT_GT(cells.size(), 100u);
  io::savePCD(out, cells);
  io::PCDMetadata meta;
  PointCloud back = io::loadPCD(out, meta);
  ASSERT_EQ(back.size(), cells.size());
  EXPECT_EQ(meta.width, uint32_t(cells.size()));
  EXPECT_EQ(back.hasIntensity(), cells.hasIntensity());
  EXPECT_TRUE(cells.hasIntensity());
  for (size_t i = 0; i < cells.size(); ++i) {
    if (back.point(i).x() != cells.point(i).x() || back.point(i).y() != cells.point(i).y() ||
        back.point(i).z() != cells.point(i).z() || back.intensity(i) != cells.intensity(i)) {
      FAIL_MSG("a cell differs after the round trip");
      break;
    }
  }
  std::remove(in.c_str());
  std::remove(out.c_str());
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
