// test_vgicp.cpp — nanoPCL's voxelized-GICP tests (lib/nanoPCL/tests/test_registration.cpp: test_vgicp_identity and
// test_vgicp_convergence of group D, test_vgicp_sparse_data of group E) at their own tolerances, re-expressed on the
// mirror's nanopcl/registration/vgicp.hpp, which this file includes FIRST (the opt-in).  Plus what the mirror adds: the
// map's accessors and host lookups, the early returns, the reference's exception for a source without covariances, a
// map that is moved.  Needs a device (tests/test_vgicp_cpp_gpu.py runs it).
#include "nanopcl/registration/vgicp.hpp"

#include <cmath>
#include <cstring>
#include <random>
#include <stdexcept>
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
static PointCloud createSparseOutdoor(size_t n, unsigned seed) {
  std::mt19937 gen(seed);
  std::uniform_real_distribution<float> xy(-50.0f, 50.0f), height(0.0f, 3.0f), prob(0.0f, 1.0f);
  PointCloud cloud;
  cloud.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    const float x = xy(gen), y = xy(gen);
    const float z = (prob(gen) < 0.7f) ? 0.1f * std::sin(x * 0.1f) : height(gen);
    cloud.add(x, y, z);
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
  Eigen::Isometry3d inv = Eigen::Isometry3d::Identity();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) inv.data()[c * 4 + r] = T.matrix()(c, r);
    inv.data()[12 + r] = -(T.matrix()(0, r) * T.matrix()(0, 3) + T.matrix()(1, r) * T.matrix()(1, 3) + T.matrix()(2, r) * T.matrix()(2, 3));
  }
  return inv;
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
static double transformError(const Eigen::Isometry3d& T1, const Eigen::Isometry3d& T2) {  // |T1 * inverse(T2) - I|
  const Eigen::Isometry3d D = T1 * inverseOf(T2);
  double s = 0.0;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      const double d = D.matrix()(r, c) - (r == c ? 1.0 : 0.0);
      s += d * d;
    }
  return std::sqrt(s);
}

// ---- D. VGICP ----
TEST(VGICP, identity) {
  PointCloud cloud = createRandomSphere(5000, 5.0f, 42);
  geometry::estimateCovariances(cloud, 20);
  registration::VoxelCorrespondence vmap(0.5f, 1e-3);
  vmap.build(cloud);
  EXPECT_GT(vmap.voxelMap().numVoxels(), size_t(1000));
  size_t found = 0;
  for (size_t i = 0; i < 100; ++i)
    found += vmap.voxelMap().lookupRegularized(nanopcl::Point(cloud.xData()[i], cloud.yData()[i], cloud.zData()[i])).has_value();
  EXPECT_EQ(found, size_t(100));  // every target point lies in a voxel of the map
  registration::AlignSettings settings;
  settings.max_iterations = 30;
  settings.min_correspondences = 5;
  const auto result = registration::alignVGICP(cloud, vmap, Eigen::Isometry3d::Identity(), settings);
  EXPECT_TRUE(result.converged || transformError(result.transform, Eigen::Isometry3d::Identity()) < 0.01);
  EXPECT_LT(transformError(result.transform, Eigen::Isometry3d::Identity()), 0.01);
}

TEST(VGICP, convergence) {
  const PointCloud target = createRandomSphere(5000, 5.0f, 42);
  registration::VoxelCorrespondence vmap(0.5f, 1e-3);
  vmap.build(target);
  const Eigen::Isometry3d gt = createRandomTransform(0.1, 0.05, 42);
  PointCloud source = transformCloud(target, inverseOf(gt));
  geometry::estimateCovariances(source, 20);
  registration::AlignSettings settings;
  settings.max_iterations = 50;
  settings.min_correspondences = 5;
  const auto result = registration::alignVGICP(source, vmap, Eigen::Isometry3d::Identity(), settings);
  EXPECT_TRUE(result.converged);
  EXPECT_GT(result.fitness, 0.1);
  EXPECT_LT(transformError(result.transform, gt), 0.2);
  // the convenience overload builds the same map for the call alone
  const auto again = registration::alignVGICP(source, target, 0.5f, Eigen::Isometry3d::Identity(), settings);
  EXPECT_EQ(again.iterations, result.iterations);
  EXPECT_EQ(std::memcmp(again.transform.data(), result.transform.data(), 16 * sizeof(double)), 0);  // the same bits
}

// ---- E. sparse data ----
TEST(VGICP, sparse_data) {
  Eigen::Isometry3d gt = Eigen::Isometry3d::Identity();
  gt.rotate(Eigen::AngleAxisd(3.0 * M_PI / 180.0, Eigen::Vector3d(0.0, 0.0, 1.0)));
  gt.pretranslate(Eigen::Vector3d(0.5, 0.25, 0.0));
  struct Case { size_t n; float voxel; };
  for (const Case t : {Case{500, 2.0f}, Case{1000, 1.5f}, Case{2000, 1.0f}, Case{5000, 1.0f}}) {
    const PointCloud target = createSparseOutdoor(t.n, 42);
    const PointCloud moved = transformCloud(target, inverseOf(gt));
    std::mt19937 gen(123);
    std::normal_distribution<float> noise(0.0f, 0.02f);
    PointCloud source;
    source.reserve(t.n);
    for (size_t i = 0; i < moved.size(); ++i) {
      const float x = moved.xData()[i] + noise(gen), y = moved.yData()[i] + noise(gen), z = moved.zData()[i] + noise(gen);
      source.add(x, y, z);
    }
    geometry::estimateCovariances(source, 20);
    registration::VoxelCorrespondence vmap(t.voxel, 1e-3);
    vmap.build(target);
    registration::AlignSettings settings;
    settings.max_iterations = 50;
    settings.min_correspondences = 3;
    const auto result = registration::alignVGICP(source, vmap, Eigen::Isometry3d::Identity(), settings);
    const Eigen::Isometry3d err = inverseOf(gt) * result.transform;
    const double t_err = std::sqrt(err.matrix()(0, 3) * err.matrix()(0, 3) + err.matrix()(1, 3) * err.matrix()(1, 3) +
                                   err.matrix()(2, 3) * err.matrix()(2, 3));
    const double c = std::min(1.0, std::max(-1.0, (err.matrix()(0, 0) + err.matrix()(1, 1) + err.matrix()(2, 2) - 1.0) / 2.0));
    const double r_err = std::acos(c) * 180.0 / M_PI;
    std::printf("  %zu points, voxel %.1f: %zu voxels, fitness %.4f, t_err %.5f m, r_err %.5f deg, %s\n", t.n, double(t.voxel),
                vmap.voxelMap().numVoxels(), result.fitness, t_err, r_err, result.converged ? "converged" : "not converged");
    if (t.n >= 1000) { EXPECT_LE(t_err, 0.1); EXPECT_LE(r_err, 1.0); }
    if (t.n >= 2000) { EXPECT_LE(t_err, 0.05); EXPECT_LE(r_err, 0.5); }
  }
}

// ---- the mirror's own ----
TEST(Mirror, map_accessors_and_host_lookups) {
  registration::VoxelDistributionMap defaults;
  EXPECT_FLOAT_EQ(defaults.resolution(), 0.5f);
  EXPECT_FLOAT_EQ(defaults.invResolution(), 2.0f);
  EXPECT_TRUE(defaults.empty());
  EXPECT_FALSE(defaults.lookup(nanopcl::Point(0.f, 0.f, 0.f)).has_value());
  registration::VoxelCorrespondence corr;
  EXPECT_FLOAT_EQ(corr.voxelMap().resolution(), 1.0f);
  EXPECT_TRUE(corr.empty());

  // one voxel of four points, one of two, one of one; a point on a face belongs to the upper voxel
  PointCloud cloud;
  cloud.add(0.1f, 0.1f, 0.1f); cloud.add(0.4f, 0.1f, 0.12f); cloud.add(0.1f, 0.4f, 0.11f); cloud.add(0.4f, 0.4f, 0.13f);
  cloud.add(-0.1f, 0.1f, 0.1f); cloud.add(-0.2f, 0.3f, 0.2f);
  cloud.add(0.5f, 0.0f, 0.0f);
  registration::VoxelDistributionMap map(0.5f, 1e-3);
  map.build(cloud);
  EXPECT_EQ(map.numVoxels(), size_t(3));
  const auto full = map.lookup(nanopcl::Point(0.25f, 0.25f, 0.25f));
  ASSERT_TRUE(full.has_value());
  EXPECT_EQ(full->num_points, 4u);
  EXPECT_TRUE(full->isValid() && full->hasFullCovariance());
  EXPECT_FLOAT_EQ(full->mean(0), 0.25f);
  EXPECT_FLOAT_EQ(full->mean(1), 0.25f);
  EXPECT_NEAR(full->covariance(0, 0), 0.0225, 1e-6);
  EXPECT_NEAR(full->covariance(0, 1), 0.0, 1e-6);
  const auto reg = map.lookupRegularized(nanopcl::Point(0.25f, 0.25f, 0.25f));
  ASSERT_TRUE(reg.has_value());
  EXPECT_NEAR(reg->covariance(0, 0) + reg->covariance(1, 1) + reg->covariance(2, 2), 2.001, 1e-5);  // eigenvalues (eps, 1, 1)
  EXPECT_LT(reg->covariance(2, 2), 0.01);                                                            // the normal is nearly z
  const auto sparse = map.lookup(nanopcl::Point(-0.3f, 0.2f, 0.4f));
  ASSERT_TRUE(sparse.has_value());
  EXPECT_EQ(sparse->num_points, 2u);
  EXPECT_TRUE(sparse->isValid());
  EXPECT_FALSE(sparse->hasFullCovariance());
  EXPECT_FLOAT_EQ(sparse->covariance(0, 0), 1e-3f);
  EXPECT_FLOAT_EQ(sparse->covariance(0, 1), 0.0f);
  const auto sparse_reg = map.lookupRegularized(nanopcl::Point(-0.3f, 0.2f, 0.4f));
  ASSERT_TRUE(sparse_reg.has_value());
  EXPECT_FLOAT_EQ(sparse_reg->covariance(1, 1), 1.0f);
  EXPECT_FLOAT_EQ(sparse_reg->covariance(1, 2), 0.0f);
  EXPECT_TRUE(map.lookup(nanopcl::Point(0.5f, 0.2f, 0.2f)).has_value());     // the face point's voxel
  EXPECT_EQ(map.lookup(nanopcl::Point(0.7f, 0.2f, 0.2f))->num_points, 1u);
  EXPECT_FALSE(map.lookup(nanopcl::Point(0.25f, 0.25f, 0.75f)).has_value()); // next to an occupied one
  EXPECT_FALSE(map.lookup(nanopcl::Point(0.25f, -0.25f, 0.25f)).has_value());

  registration::VoxelDistributionMap moved(std::move(map));                  // the handle moves with its records
  EXPECT_EQ(moved.numVoxels(), size_t(3));
  EXPECT_TRUE(map.empty());
  EXPECT_TRUE(map.handle() == nullptr);
  EXPECT_TRUE(moved.lookup(nanopcl::Point(0.25f, 0.25f, 0.25f)).has_value());
  moved.build(PointCloud());                                                 // an empty cloud empties the map
  EXPECT_TRUE(moved.empty());
}

TEST(Mirror, early_returns_and_the_missing_covariances) {
  PointCloud target = createRandomSphere(500, 2.0f, 7);
  PointCloud source = target;  // no covariances
  const PointCloud empty;
  registration::VoxelCorrespondence vmap(0.5f, 1e-3), none(0.5f, 1e-3);
  vmap.build(target);
  Eigen::Isometry3d guess = Eigen::Isometry3d::Identity();
  guess.pretranslate(Eigen::Vector3d(1.0, 2.0, 3.0));
  for (const auto& r : {registration::alignVGICP(empty, vmap, guess), registration::alignVGICP(source, none, guess),
                        registration::alignVGICP(empty, target, 1.0f, guess), registration::alignVGICP(source, empty, 1.0f, guess)}) {
    EXPECT_FALSE(r.converged);                                               // before the covariances are asked for
    EXPECT_EQ(r.iterations, size_t(0));
    EXPECT_EQ(r.fitness, 0.0);
    EXPECT_TRUE(std::isinf(r.rmse));
    EXPECT_FALSE(r.covariance.has_value());
    EXPECT_EQ(std::memcmp(r.transform.data(), guess.data(), 16 * sizeof(double)), 0);
  }
  bool thrown = false;
  try {
    (void)registration::alignVGICP(source, vmap);
  } catch (const std::runtime_error& e) {
    thrown = std::string(e.what()) == "alignVGICP: source must have covariances. Call geometry::estimateCovariances() first.";
  }
  EXPECT_TRUE(thrown);
  EXPECT_THROW((void)registration::alignVGICP(source, target), std::runtime_error);
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
