// test_registration.cpp — nanoPCL's registration tests (lib/nanoPCL/tests/test_registration.cpp), its convergence group B
// and its stability group C at their own tolerances, re-expressed on the mirror's nanopcl/registration.hpp.  The VGICP
// cases have no counterpart (alignVGICP is declared deleted); groups A and D test types the mirror does not carry and are
// covered in tests/test_reg_restate.py.  Plus what the mirror adds: the reference's exceptions for a missing channel, the
// result's helpers, the deleted overloads.  Needs a device (tests/test_register_cpp_gpu.py runs it).
#include <cmath>
#include <random>
#include <stdexcept>
#include <type_traits>
#include <utility>

#include "mini_test.hpp"
#include "nanopcl/core.hpp"

using nanopcl::PointCloud;
namespace geometry = nanopcl::geometry;
namespace registration = nanopcl::registration;

static PointCloud createRandomSphere(size_t n, float radius = 1.0f, unsigned seed = 42) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> dist(-1.0f, 1.0f);
  PointCloud cloud;
  cloud.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    float x = dist(rng), y = dist(rng), z = dist(rng);
    float norm = std::sqrt(x * x + y * y + z * z);
    if (norm < 1e-6f) { x = 1.0f; norm = 1.0f; }
    cloud.add(radius * x / norm, radius * y / norm, radius * z / norm);
  }
  return cloud;
}
static PointCloud createRandomPlane(size_t n, unsigned seed = 42) {  // z = 0.1 x + 0.2 y + noise
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> xy_dist(-5.0f, 5.0f), noise_dist(-0.01f, 0.01f);
  PointCloud cloud;
  cloud.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    const float x = xy_dist(rng), y = xy_dist(rng);
    cloud.add(x, y, 0.1f * x + 0.2f * y + 0.0f + noise_dist(rng));
  }
  return cloud;
}
static Eigen::Isometry3d createRandomTransform(double max_translation, double max_rotation_rad, unsigned seed = 123) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> t_dist(-max_translation, max_translation), r_dist(-max_rotation_rad, max_rotation_rad);
  Eigen::Isometry3d T = Eigen::Isometry3d::Identity();
  const double tx = t_dist(rng), ty = t_dist(rng), tz = t_dist(rng);
  T.pretranslate(Eigen::Vector3d(tx, ty, tz));
  const double ax = r_dist(rng), ay = r_dist(rng), az = r_dist(rng);
  const double angle = std::sqrt(ax * ax + ay * ay + az * az);
  if (angle > 1e-6) T.rotate(Eigen::AngleAxisd(angle, Eigen::Vector3d(ax / angle, ay / angle, az / angle)));
  return T;
}
static Eigen::Isometry3d inverseOf(const Eigen::Isometry3d& T) {  // [RT, -RT t]
  double m[16] = {};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m[c * 4 + r] = T.matrix()(c, r);
    m[12 + r] = -(T.matrix()(0, r) * T.matrix()(0, 3) + T.matrix()(1, r) * T.matrix()(1, 3) + T.matrix()(2, r) * T.matrix()(2, 3));
  }
  m[15] = 1.0;
  Eigen::Isometry3d inv = Eigen::Isometry3d::Identity();
  for (int i = 0; i < 16; ++i) inv.data()[i] = m[i];
  return inv;
}
static Eigen::Isometry3d translationOf(double x, double y, double z) {
  Eigen::Isometry3d T = Eigen::Isometry3d::Identity();
  T.pretranslate(Eigen::Vector3d(x, y, z));
  return T;
}
static PointCloud transformCloud(const PointCloud& cloud, const Eigen::Isometry3d& T) {
  PointCloud out;
  out.reserve(cloud.size());
  for (size_t i = 0; i < cloud.size(); ++i) {
    const Eigen::Vector3d p = T * Eigen::Vector3d(cloud.xData()[i], cloud.yData()[i], cloud.zData()[i]);
    out.add(float(p[0]), float(p[1]), float(p[2]));
  }
  return out;
}
// Frobenius norm of T1 * inverse(T2) - I
static double transformError(const Eigen::Isometry3d& T1, const Eigen::Isometry3d& T2) {
  const Eigen::Isometry3d D = T1 * inverseOf(T2);
  double s = 0.0;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      const double d = D.matrix()(r, c) - (r == c ? 1.0 : 0.0);
      s += d * d;
    }
  return std::sqrt(s);
}

// ---- B. convergence ----
TEST(Convergence, icp_identity) {
  const PointCloud cloud = createRandomSphere(500);
  const auto result = registration::alignICP(cloud, cloud);
  EXPECT_TRUE(result.converged);
  EXPECT_NEAR(transformError(result.transform, Eigen::Isometry3d::Identity()), 0.0, 1e-6);
}

TEST(Convergence, icp_simple_translation) {
  const PointCloud target = createRandomSphere(500);
  const Eigen::Isometry3d gt = translationOf(0.5, 0.0, 0.0);
  const PointCloud source = transformCloud(target, inverseOf(gt));
  registration::AlignSettings settings;
  settings.max_correspondence_dist = 1.0f;
  settings.max_iterations = 100;
  const auto result = registration::alignICP(source, target, Eigen::Isometry3d::Identity(), settings);
  EXPECT_TRUE(result.converged);
  EXPECT_LT(transformError(result.transform, gt), 0.01);
}

TEST(Convergence, icp_rotation_translation) {
  const PointCloud target = createRandomSphere(1000);
  const Eigen::Isometry3d gt = createRandomTransform(0.3, 0.15, 42);
  const PointCloud source = transformCloud(target, inverseOf(gt));
  registration::AlignSettings settings;
  settings.max_correspondence_dist = 1.0f;
  settings.max_iterations = 100;
  const auto result = registration::alignICP(source, target, Eigen::Isometry3d::Identity(), settings);
  EXPECT_TRUE(result.converged);
  EXPECT_LT(transformError(result.transform, gt), 0.05);
}

TEST(Convergence, plane_icp) {
  PointCloud target = createRandomPlane(1000);
  geometry::estimateNormals(target, 20);
  const Eigen::Isometry3d gt = createRandomTransform(0.2, 0.1, 42);
  const PointCloud source = transformCloud(target, inverseOf(gt));
  registration::AlignSettings settings;
  settings.max_correspondence_dist = 1.0f;
  settings.max_iterations = 50;
  const auto result = registration::alignPlaneICP(source, target, Eigen::Isometry3d::Identity(), settings);
  EXPECT_TRUE(result.converged);
  EXPECT_LT(transformError(result.transform, gt), 0.02);
}

TEST(Convergence, gicp) {
  PointCloud target = createRandomSphere(1000);
  geometry::estimateCovariances(target, 20);
  const Eigen::Isometry3d gt = createRandomTransform(0.2, 0.1, 42);
  PointCloud source = transformCloud(target, inverseOf(gt));
  geometry::estimateCovariances(source, 20);
  registration::AlignSettings settings;
  settings.max_correspondence_dist = 1.0f;
  settings.max_iterations = 50;
  settings.covariance_epsilon = 1e-3;
  const auto result = registration::alignGICP(source, target, Eigen::Isometry3d::Identity(), settings);
  EXPECT_TRUE(result.converged);
  EXPECT_LT(transformError(result.transform, gt), 0.02);
}

TEST(Convergence, gicp_identity) {
  PointCloud cloud = createRandomSphere(500);
  geometry::estimateCovariances(cloud, 20);
  const auto result = registration::alignGICP(cloud, cloud);
  EXPECT_TRUE(result.converged);
  EXPECT_NEAR(transformError(result.transform, Eigen::Isometry3d::Identity()), 0.0, 1e-5);
}

// ---- C. stability ----
TEST(Stability, empty_cloud) {
  const PointCloud empty;
  const PointCloud target = createRandomSphere(100);
  const auto result = registration::alignICP(empty, target);
  EXPECT_FALSE(result.converged);
  EXPECT_EQ(result.iterations, 0u);
  EXPECT_FALSE(registration::alignPlaneICP(target, empty).converged);  // before the channels are looked at
  EXPECT_FALSE(registration::alignGICP(empty, target).converged);
}

TEST(Stability, sparse_cloud) {
  PointCloud source, target;
  source.add(0, 0, 0);
  source.add(1, 0, 0);
  source.add(0, 1, 0);
  target.add(0.1f, 0, 0);
  target.add(1.1f, 0, 0);
  target.add(0.1f, 1, 0);
  registration::AlignSettings settings;
  settings.min_correspondences = 10;
  const auto result = registration::alignICP(source, target, Eigen::Isometry3d::Identity(), settings);
  EXPECT_FALSE(result.converged);
  EXPECT_FALSE(result.covariance.has_value());
}

TEST(Stability, bad_initial_guess) {
  const PointCloud target = createRandomSphere(500);
  const PointCloud source = transformCloud(target, inverseOf(translationOf(0.1, 0.0, 0.0)));
  registration::AlignSettings settings;
  settings.max_correspondence_dist = 0.5f;
  settings.max_iterations = 50;
  const auto result = registration::alignICP(source, target, translationOf(10.0, 10.0, 10.0), settings);
  EXPECT_FALSE(result.converged);  // nothing within 0.5 m: fewer than min_correspondences
  EXPECT_EQ(result.fitness, 0.0);
}

TEST(Stability, partial_overlap) {
  const PointCloud target = createRandomSphere(500, 1.0f, 42);
  const PointCloud source = transformCloud(createRandomSphere(500, 1.0f, 43), translationOf(1.5, 0.0, 0.0));
  registration::AlignSettings settings;
  settings.max_correspondence_dist = 0.3f;
  settings.max_iterations = 50;
  const auto result = registration::alignICP(source, target, Eigen::Isometry3d::Identity(), settings);
  EXPECT_LT(result.fitness, 1.0);
}

// ---- what the mirror adds ----
TEST(Mirror, missing_channels_throw_as_in_the_reference) {
  PointCloud target = createRandomSphere(100);
  const PointCloud source = createRandomSphere(100, 1.0f, 43);
  EXPECT_THROW((void)registration::alignPlaneICP(source, target), std::runtime_error);
  EXPECT_THROW((void)registration::alignGICP(source, target), std::runtime_error);
  geometry::estimateCovariances(target, 20);
  EXPECT_THROW((void)registration::alignGICP(source, target), std::runtime_error);   // the source's are missing
  registration::AlignSettings settings;
  settings.max_correspondence_dist = -1.0f;
  EXPECT_THROW((void)registration::alignICP(source, target, Eigen::Isometry3d::Identity(), settings), std::runtime_error);
}

TEST(Mirror, result_helpers) {
  const PointCloud target = createRandomSphere(500);
  const PointCloud source = transformCloud(target, inverseOf(translationOf(0.1, 0.0, 0.0)));
  const auto result = registration::alignICP(source, target);
  EXPECT_TRUE(result.success());
  EXPECT_FALSE(result.success(1.5));
  ASSERT_TRUE(result.covariance.has_value());
  const auto info = result.informationMatrix();
  ASSERT_TRUE(info.has_value());
  const registration::Matrix6d I = (*info) * (*result.covariance);
  EXPECT_LT((I - registration::Matrix6d::Identity()).norm(), 1e-9);
  EXPECT_NEAR((*info)(0, 0), 500.0, 1e-6);  // the ICP factor's H(0, 0) is the inlier count
}

// alignVGICP is refused at compile time
template <typename Second, typename = void>
struct HasVGICP : std::false_type {};
template <typename Second>
struct HasVGICP<Second, std::void_t<decltype(registration::alignVGICP(std::declval<const PointCloud&>(), std::declval<Second>()))>>
    : std::true_type {};
TEST(Mirror, vgicp_overloads_are_deleted) {
  EXPECT_FALSE(HasVGICP<const PointCloud&>::value);
  EXPECT_FALSE(HasVGICP<const registration::VoxelCorrespondence&>::value);
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
