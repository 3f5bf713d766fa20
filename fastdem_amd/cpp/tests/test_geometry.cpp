// test_geometry.cpp — nanoPCL's normal / covariance estimation tests (lib/nanoPCL/tests/test_geometry.cpp, its seventeen
// cases at its own tolerances) re-expressed on the mirror's nanopcl/geometry/normal_estimation.hpp.  The cases that hand
// over a pre-built search::KdTree call the plain overload: the mirror has no KdTree.  Plus what the mirror adds: the
// refusal of more than 64 neighbours, and the radius overloads being deleted rather than converted.  Needs a device: the
// estimation runs there (tests/test_normals_cpp_gpu.py runs it).
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <type_traits>
#include <utility>

#include "mini_test.hpp"
#include "nanopcl/core.hpp"

using nanopcl::Normal4;
using nanopcl::Point;
using nanopcl::PointCloud;
namespace geometry = nanopcl::geometry;

static PointCloud createPlaneXY(int n = 10, float z = 0.0f) {
  PointCloud cloud;
  for (int x = 0; x < n; ++x)
    for (int y = 0; y < n; ++y) cloud.add(float(x), float(y), z);
  return cloud;
}
static PointCloud createPlaneXZ(int n = 10, float y = 0.0f) {
  PointCloud cloud;
  for (int x = 0; x < n; ++x)
    for (int z = 0; z < n; ++z) cloud.add(float(x), y, float(z));
  return cloud;
}
static PointCloud createTiltedPlane(int n = 10) {  // z = 0.5 x + 0.3 y: the normal is along (-0.5, -0.3, 1)
  PointCloud cloud;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const float x = float(i), y = float(j);
      cloud.add(x, y, 0.5f * x + 0.3f * y);
    }
  return cloud;
}
static PointCloud createSparseCloud() {  // two points: not enough for a PCA
  PointCloud cloud;
  cloud.add(0, 0, 0);
  cloud.add(1, 0, 0);
  return cloud;
}
static PointCloud createCollinearPoints() {
  PointCloud cloud;
  for (int i = 0; i < 10; ++i) cloud.add(float(i), 0, 0);
  return cloud;
}

static float norm3(const Normal4& n) { return std::sqrt(n.x() * n.x() + n.y() * n.y() + n.z() * n.z()); }
static float dot3(const Normal4& n, const Eigen::Vector3f& v) { return n.x() * v[0] + n.y() * v[1] + n.z() * v[2]; }
// eigenvalues of a symmetric 3 x 3, ascending (cyclic Jacobi in double: the mirror's mini Eigen has no solver)
static void eigenvalues(const Eigen::Matrix3f& c, double w[3]) {
  double a[3][3];
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s) a[r][s] = 0.5 * (double(c(r, s)) + double(c(s, r)));
  for (int sweep = 0; sweep < 50; ++sweep)
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (std::fabs(a[p][q]) < 1e-300) continue;
        const double theta = 0.5 * std::atan2(2.0 * a[p][q], a[q][q] - a[p][p]);
        const double cs = std::cos(theta), sn = std::sin(theta);
        for (int k = 0; k < 3; ++k) {
          const double kp = a[k][p], kq = a[k][q];
          a[k][p] = cs * kp - sn * kq;
          a[k][q] = sn * kp + cs * kq;
        }
        for (int k = 0; k < 3; ++k) {
          const double pk = a[p][k], qk = a[q][k];
          a[p][k] = cs * pk - sn * qk;
          a[q][k] = sn * pk + cs * qk;
        }
      }
  w[0] = a[0][0]; w[1] = a[1][1]; w[2] = a[2][2];
  std::sort(w, w + 3);
}

// ---- Normal Estimation ----
TEST(Normals, plane_xy) {
  auto cloud = createPlaneXY(5, 0.0f);
  geometry::estimateNormals(cloud, 10);
  ASSERT_TRUE(cloud.hasNormal());
  const Normal4 n = cloud.normal(12);  // (2, 2) of the 5 x 5 lattice: away from the border
  EXPECT_LT(std::fabs(std::fabs(n.x()) - 0.0f), 0.1f);
  EXPECT_LT(std::fabs(std::fabs(n.y()) - 0.0f), 0.1f);
  EXPECT_LT(std::fabs(std::fabs(n.z()) - 1.0f), 0.1f);
}

TEST(Normals, plane_xz) {
  auto cloud = createPlaneXZ(5, 0.0f);
  geometry::estimateNormals(cloud, 10);
  ASSERT_TRUE(cloud.hasNormal());
  const Normal4 n = cloud.normal(12);
  EXPECT_LT(std::fabs(std::fabs(n.x()) - 0.0f), 0.1f);
  EXPECT_LT(std::fabs(std::fabs(n.y()) - 1.0f), 0.1f);
  EXPECT_LT(std::fabs(std::fabs(n.z()) - 0.0f), 0.1f);
}

TEST(Normals, plane_arbitrary) {
  auto cloud = createTiltedPlane(5);
  geometry::estimateNormals(cloud, 10);
  ASSERT_TRUE(cloud.hasNormal());
  Eigen::Vector3f expected(-0.5f, -0.3f, 1.0f);
  const float len = expected.norm();
  for (int i = 0; i < 3; ++i) expected[i] /= len;
  const Normal4 n = cloud.normal(12);
  EXPECT_LT(std::fabs(std::fabs(dot3(n, expected)) - 1.0f), 0.1f);
}

TEST(Normals, viewpoint_orientation) {
  auto cloud = createPlaneXY(5, 0.0f);
  const Point viewpoint(2.0f, 2.0f, 10.0f);  // above the plane
  geometry::estimateNormals(cloud, 10, viewpoint);
  const Normal4 n = cloud.normal(12);
  const Eigen::Vector3f to_viewpoint = viewpoint - Eigen::Vector3f(cloud.point(12));
  EXPECT_TRUE(dot3(n, to_viewpoint) > 0);
}

TEST(Normals, viewpoint_below) {
  auto cloud = createPlaneXY(5, 0.0f);
  geometry::estimateNormals(cloud, 10, Point(2.0f, 2.0f, -10.0f));
  const Normal4 n = cloud.normal(12);
  EXPECT_TRUE(n.z() < 0);
}

TEST(Normals, sparse_cloud) {
  auto cloud = createSparseCloud();
  geometry::estimateNormals(cloud, 10);
  ASSERT_TRUE(cloud.hasNormal());
  const Normal4 n0 = cloud.normal(0), n1 = cloud.normal(1);
  EXPECT_LT(std::fabs(norm3(n0) - 0.0f), 1e-5f);
  EXPECT_LT(std::fabs(norm3(n1) - 0.0f), 1e-5f);
}

TEST(Normals, with_external_kdtree) {  // (the plain overload: the mirror has no KdTree)
  auto cloud = createPlaneXY(5, 0.0f);
  geometry::estimateNormals(cloud, 10);
  ASSERT_TRUE(cloud.hasNormal());
  const Normal4 n = cloud.normal(12);
  EXPECT_LT(std::fabs(std::fabs(n.z()) - 1.0f), 0.1f);
}

// ---- Covariance Estimation ----
TEST(Covariances, planar) {
  auto cloud = createPlaneXY(5, 0.0f);
  geometry::estimateCovariances(cloud, 10);
  ASSERT_TRUE(cloud.hasCovariance());
  double w[3];
  eigenvalues(cloud.covariance(12), w);
  EXPECT_LT(std::fabs(w[0] - 1e-3), 1e-4);  // the GICP regularisation: (epsilon, 1, 1)
  EXPECT_LT(std::fabs(w[1] - 1.0), 0.1);
  EXPECT_LT(std::fabs(w[2] - 1.0), 0.1);
}

TEST(Covariances, gicp_regularization) {
  auto cloud = createPlaneXY(5, 0.0f);
  geometry::estimateCovariances(cloud, 10);
  const Eigen::Matrix3f cov = cloud.covariance(12);
  EXPECT_LT(std::fabs(cov(0, 1) - cov(1, 0)), 1e-6f);
  EXPECT_LT(std::fabs(cov(0, 2) - cov(2, 0)), 1e-6f);
  EXPECT_LT(std::fabs(cov(1, 2) - cov(2, 1)), 1e-6f);
  double w[3];
  eigenvalues(cov, w);
  for (int i = 0; i < 3; ++i) EXPECT_TRUE(w[i] >= 0);
}

TEST(Covariances, invalid_returns_identity) {
  auto cloud = createSparseCloud();
  geometry::estimateCovariances(cloud, 10);
  ASSERT_TRUE(cloud.hasCovariance());
  const Eigen::Matrix3f cov = cloud.covariance(0);
  EXPECT_LT(std::fabs(cov(0, 0) - 1.0f), 1e-5f);
  EXPECT_LT(std::fabs(cov(1, 1) - 1.0f), 1e-5f);
  EXPECT_LT(std::fabs(cov(2, 2) - 1.0f), 1e-5f);
  EXPECT_LT(std::fabs(cov(0, 1) - 0.0f), 1e-5f);
}

TEST(Covariances, with_external_kdtree) {
  auto cloud = createPlaneXY(5, 0.0f);
  geometry::estimateCovariances(cloud, 10);
  ASSERT_TRUE(cloud.hasCovariance());
  const Eigen::Matrix3f cov = cloud.covariance(12);
  EXPECT_TRUE(cov(0, 0) + cov(1, 1) + cov(2, 2) > 0);
}

// ---- Combined ----
TEST(Combined, single_pass) {
  auto cloud1 = createPlaneXY(5, 0.0f);
  auto cloud2 = createPlaneXY(5, 0.0f);
  geometry::estimateNormalsCovariances(cloud1, 10);
  geometry::estimateNormals(cloud2, 10);
  geometry::estimateCovariances(cloud2, 10);
  ASSERT_TRUE(cloud1.hasNormal());
  ASSERT_TRUE(cloud1.hasCovariance());
  for (size_t i = 0; i < cloud1.size(); ++i) {
    const Normal4 n1 = cloud1.normal(i), n2 = cloud2.normal(i);
    const Normal4 dn(n1.x() - n2.x(), n1.y() - n2.y(), n1.z() - n2.z(), 0.0f);
    EXPECT_LT(std::fabs(norm3(dn) - 0.0f), 1e-5f);
    const Eigen::Matrix3f c1 = cloud1.covariance(i), c2 = cloud2.covariance(i);
    float ss = 0.0f;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) ss += (c1(r, c) - c2(r, c)) * (c1(r, c) - c2(r, c));
    EXPECT_LT(std::fabs(std::sqrt(ss) - 0.0f), 1e-5f);
  }
}

TEST(Combined, with_external_kdtree) {
  auto cloud = createPlaneXY(5, 0.0f);
  geometry::estimateNormalsCovariances(cloud, 10);
  EXPECT_TRUE(cloud.hasNormal());
  EXPECT_TRUE(cloud.hasCovariance());
}

// ---- Edge Cases ----
TEST(EdgeCases, empty_cloud) {
  PointCloud cloud;
  geometry::estimateNormals(cloud, 10);
  EXPECT_FALSE(cloud.hasNormal());
  geometry::estimateCovariances(cloud, 10);
  EXPECT_FALSE(cloud.hasCovariance());
  geometry::estimateNormalsCovariances(cloud, 10);
  EXPECT_FALSE(cloud.hasNormal());
  EXPECT_FALSE(cloud.hasCovariance());
}

TEST(EdgeCases, single_point) {
  PointCloud cloud;
  cloud.add(1, 2, 3);
  geometry::estimateNormals(cloud, 10);
  ASSERT_TRUE(cloud.hasNormal());
  EXPECT_LT(std::fabs(norm3(cloud.normal(0)) - 0.0f), 1e-5f);
}

TEST(EdgeCases, collinear_points) {
  auto cloud = createCollinearPoints();
  geometry::estimateNormals(cloud, 5);
  EXPECT_TRUE(cloud.hasNormal());  // a degenerate plane: no crash, the channel is set
}

TEST(EdgeCases, normal_unit_length) {
  auto cloud = createPlaneXY(5, 0.0f);
  geometry::estimateNormals(cloud, 10);
  for (size_t i = 0; i < cloud.size(); ++i) {
    const float len = norm3(cloud.normal(i));
    EXPECT_TRUE(len < 1e-5f || std::fabs(len - 1.0f) < 1e-5f);
  }
}

// ---- what the mirror adds ----
TEST(Mirror, more_than_64_neighbours_throw) {
  auto cloud = createPlaneXY(10, 0.0f);
  EXPECT_THROW(geometry::estimateNormals(cloud, 65), std::runtime_error);
  EXPECT_THROW(geometry::estimateCovariances(cloud, -1), std::runtime_error);  // every point: 100 of them
  EXPECT_NO_THROW(geometry::estimateNormalsCovariances(cloud, 64));
}

// a radius is refused at compile time, never converted to a neighbour count
template <typename K, typename = void>
struct Callable : std::false_type {};
template <typename K>
struct Callable<K, std::void_t<decltype(geometry::estimateNormals(std::declval<PointCloud&>(), std::declval<K>()))>>
    : std::true_type {};
TEST(Mirror, radius_overloads_are_deleted) {
  EXPECT_TRUE(Callable<int>::value);
  EXPECT_FALSE(Callable<float>::value);
}

int main(int argc, char** argv) { return mini::run(argc > 1 ? argv[1] : nullptr); }
