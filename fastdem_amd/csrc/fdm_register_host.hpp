// fdm_register_host.hpp — the small algebra of cloud registration that stays on the host, all in double: the packed
// quadratic model, the damped 6 x 6 solve, se3Exp, the termination criteria, the result and the rule for its covariance.
// Plain C++17 with no device code and no HIP header, so that a CPU-only program can include it (tests build one under
// the sanitizers).  The device side is fdm_register.hpp, the driver fdm_engine_register.inl.
//
// Reference being reproduced: nanoPCL registration — iterative_solver.hpp:96-219 (the loop and the three result
// makers), optimizers/lm_optimizer.hpp:98-103 (computeDelta: the only optimizer call the loop makes, so lambda stays
// 1e-3), criteria.hpp:40-68, linearizers/linearizer.hpp:42-53 (the packing), core/lie.hpp:39-59, 91-104, 130-148.
//
// The twist is [v; omega]: se3Exp takes the first three as v and the last three as omega, and the factors' Jacobians
// agree.  criteria.hpp calls tail<3>() "translation" and head<3>() "rotation": THE NAMES ARE SWAPPED relative to that
// layout — translation_eps bounds |omega| and rotation_eps bounds |v|.  That is the reference's behaviour and it is
// kept as written.
//
// DEVIATION (include/fdm_engine.h).  The reference's covariance is ldlt().solve(I) whenever Eigen's
// pivoted LDLT reports isPositive(), which it also does for a semidefinite H (plane ICP on a planar target: rank 3),
// solving with the near-zero pivots zeroed.  Here the covariance exists only when an unpivoted Cholesky of the
// undamped H finds every pivot above n_source * 2^-52 * max diag(H); it is then inverse(H).
#pragma once

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace fdm {
namespace reg {

constexpr double kLambda = 1e-3;  // LMOptimizer::init_lambda; never adapted

// one linearization: upper-triangular row-major H (21), b (6), the error and the inlier count
struct Model {
  double H[21] = {};
  double b[6] = {};
  double error = 0.0;
  uint64_t num_inliers = 0;
};

struct Mat6 {
  double a[6][6];
};

// toFullHessian (linearizer.hpp:42-53)
inline Mat6 full_hessian(const double* h) {
  Mat6 M;
  int idx = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      M.a[r][c] = h[idx];
      M.a[c][r] = h[idx];
      ++idx;
    }
  return M;
}

// delta = (H + lambda I)^-1 (-b) by Gaussian elimination with partial pivoting (the reference: Eigen's LDLT; the two
// differ by rounding only).  A pivot of exactly zero leaves a delta that is not finite: nothing converges on it.
inline void compute_delta(const Mat6& H, const double* b, double lambda, double* delta) {
  double A[6][7];
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) A[r][c] = H.a[r][c] + (r == c ? lambda : 0.0);
    A[r][6] = -b[r];
  }
  for (int k = 0; k < 6; ++k) {
    int piv = k;
    for (int r = k + 1; r < 6; ++r)
      if (std::fabs(A[r][k]) > std::fabs(A[piv][k])) piv = r;
    if (piv != k)
      for (int c = 0; c < 7; ++c) {
        const double t = A[k][c];
        A[k][c] = A[piv][c];
        A[piv][c] = t;
      }
    for (int r = k + 1; r < 6; ++r) {
      const double f = A[r][k] / A[k][k];
      for (int c = k; c < 7; ++c) A[r][c] -= f * A[k][c];
    }
  }
  for (int r = 5; r >= 0; --r) {
    double s = A[r][6];
    for (int c = r + 1; c < 6; ++c) s -= A[r][c] * delta[c];
    delta[r] = s / A[r][r];
  }
}

// A rigid transform: rotation row-major, translation.  (The C ABI carries 16 column-major doubles.)
struct Rigid {
  double R[3][3];
  double t[3];
};
inline Rigid rigid_identity() { return Rigid{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, {0, 0, 0}}; }
inline Rigid rigid_from_colmajor(const double* m) {
  Rigid T;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T.R[r][c] = m[c * 4 + r];
    T.t[r] = m[12 + r];
  }
  return T;
}
inline void rigid_to_colmajor(const Rigid& T, double* m) {
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) m[c * 4 + r] = r == 3 ? (c == 3 ? 1.0 : 0.0) : (c == 3 ? T.t[r] : T.R[r][c]);
}
// A * B (Isometry3d's product: the linear parts multiply, the translation is A.R * B.t + A.t)
inline Rigid rigid_mul(const Rigid& A, const Rigid& B) {
  Rigid C;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) C.R[r][c] = (A.R[r][0] * B.R[0][c] + A.R[r][1] * B.R[1][c]) + A.R[r][2] * B.R[2][c];
    C.t[r] = ((A.R[r][0] * B.t[0] + A.R[r][1] * B.t[1]) + A.R[r][2] * B.t[2]) + A.t[r];
  }
  return C;
}

// se3Exp (lie.hpp:130-148): R = so3Exp(omega) — the identity below |omega| = 1e-10, otherwise Eigen's
// AngleAxis::toRotationMatrix — and t = leftJacobian(omega) * v with the axis-form coefficients
// c1 = (1 - cos) / theta, c2 = (theta - sin) / theta over the unit axis' skew matrix (lie.hpp:50-58).
inline Rigid se3_exp(const double* xi) {
  const double v[3] = {xi[0], xi[1], xi[2]}, w[3] = {xi[3], xi[4], xi[5]};
  Rigid T = rigid_identity();
  const double theta = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (theta < 1e-10) {
    for (int r = 0; r < 3; ++r) T.t[r] = v[r];
    return T;
  }
  const double a[3] = {w[0] / theta, w[1] / theta, w[2] / theta};
  const double s = std::sin(theta), c = std::cos(theta);
  const double sa[3] = {s * a[0], s * a[1], s * a[2]};
  const double ca[3] = {(1.0 - c) * a[0], (1.0 - c) * a[1], (1.0 - c) * a[2]};
  double tmp = ca[0] * a[1];
  T.R[0][1] = tmp - sa[2];
  T.R[1][0] = tmp + sa[2];
  tmp = ca[0] * a[2];
  T.R[0][2] = tmp + sa[1];
  T.R[2][0] = tmp - sa[1];
  tmp = ca[1] * a[2];
  T.R[1][2] = tmp - sa[0];
  T.R[2][1] = tmp + sa[0];
  for (int r = 0; r < 3; ++r) T.R[r][r] = ca[r] * a[r] + c;
  const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
  const double c1 = (1.0 - c) / theta, c2 = (theta - s) / theta;
  double J[3][3];
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) {
      const double kk = (K[r][0] * K[0][q] + K[r][1] * K[1][q]) + K[r][2] * K[2][q];
      J[r][q] = ((r == q ? 1.0 : 0.0) + c1 * K[r][q]) + c2 * kk;
    }
  for (int r = 0; r < 3; ++r) T.t[r] = (J[r][0] * v[0] + J[r][1] * v[1]) + J[r][2] * v[2];
  return T;
}

struct Criteria {
  int max_iterations = 50;
  uint64_t min_correspondences = 10;
  double translation_eps = 1e-4, rotation_eps = 1e-4, relative_error_eps = 1e-6;
  // criteria.hpp:40-54, names as written there (swapped: see the file comment)
  bool converged(const double* delta, double prev_error, double curr_error) const {
    const double dt = std::sqrt(delta[3] * delta[3] + delta[4] * delta[4] + delta[5] * delta[5]);  // tail<3>
    const double dr = std::sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);  // head<3>
    const bool is_stable = dt < translation_eps && dr < rotation_eps;
    const double rel_change = prev_error > 0 ? std::fabs(prev_error - curr_error) / prev_error : 0.0;
    return is_stable || rel_change < relative_error_eps;
  }
};

struct Result {
  Rigid T = rigid_identity();
  double fitness = 0.0;
  double rmse = std::numeric_limits<double>::infinity();
  uint64_t iterations = 0;
  bool converged = false;
  bool has_covariance = false;
  double covariance[36] = {};  // row-major (symmetric)
};

// inverse(H) where an unpivoted Cholesky finds every pivot above n_source * 2^-52 * max diag(H) (the file comment)
inline bool covariance_of(const Mat6& H, uint64_t n_source, double* cov36) {
  double top = 0.0;
  for (int r = 0; r < 6; ++r) top = H.a[r][r] > top ? H.a[r][r] : top;
  const double floor_ = double(n_source) * 2.220446049250313e-16 * top;
  double L[6][6] = {};
  for (int j = 0; j < 6; ++j) {
    double d = H.a[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > floor_) || !std::isfinite(d)) return false;
    L[j][j] = std::sqrt(d);
    for (int r = j + 1; r < 6; ++r) {
      double s = H.a[r][j];
      for (int k = 0; k < j; ++k) s -= L[r][k] * L[j][k];
      L[r][j] = s / L[j][j];
    }
  }
  for (int c = 0; c < 6; ++c) {  // L y = e_c, LT x = y
    double y[6], x[6];
    for (int r = 0; r < 6; ++r) {
      double s = r == c ? 1.0 : 0.0;
      for (int k = 0; k < r; ++k) s -= L[r][k] * y[k];
      y[r] = s / L[r][r];
    }
    for (int r = 5; r >= 0; --r) {
      double s = y[r];
      for (int k = r + 1; k < 6; ++k) s -= L[k][r] * x[k];
      x[r] = s / L[r][r];
    }
    for (int r = 0; r < 6; ++r) cov36[r * 6 + c] = x[r];
  }
  return true;
}

inline Result failed_result(const Rigid& T, int iterations) {  // makeFailedResult
  Result r;
  r.T = T;
  r.iterations = uint64_t(iterations);
  return r;
}
// makeSuccessResult / makeResult: the statistics of `model`, the covariance of the undamped H
inline Result model_result(const Rigid& T, const Model& model, int iterations, bool converged, const Mat6& H,
                           uint64_t n_points) {
  Result r;
  r.T = T;
  r.fitness = n_points > 0 ? double(model.num_inliers) / double(n_points) : 0.0;
  // makeSuccessResult divides without a guard (no inliers and min_correspondences = 0: 0 / 0, a NaN); makeResult guards
  r.rmse = converged || model.num_inliers > 0 ? std::sqrt(2.0 * model.error / double(model.num_inliers))
                                              : std::numeric_limits<double>::infinity();
  r.iterations = uint64_t(iterations);
  r.converged = converged;
  r.has_covariance = covariance_of(H, n_points, r.covariance);
  return r;
}

// IterativeSolver<LMOptimizer>::solve (iterative_solver.hpp:96-149).  linearize(T, model) fills one model at T and
// returns 0, or an error code that ends the loop (*rc).
template <class Linearize>
Result solve(uint64_t n_points, const Rigid& initial_guess, const Criteria& crit, Linearize&& linearize, int* rc) {
  *rc = 0;
  if (n_points == 0) return failed_result(initial_guess, 0);
  Rigid T = initial_guess;
  double prev_error = DBL_MAX;
  Mat6 last_H = {};
  Model last_model;
  for (int iter = 0; iter < crit.max_iterations; ++iter) {
    Model model;
    if ((*rc = linearize(T, model)) != 0) return failed_result(T, iter);
    last_model = model;
    if (model.num_inliers < crit.min_correspondences) return failed_result(T, iter);
    const Mat6 H = full_hessian(model.H);
    last_H = H;
    double delta[6];
    compute_delta(H, model.b, kLambda, delta);
    const Rigid new_T = rigid_mul(se3_exp(delta), T);
    if (crit.converged(delta, prev_error, model.error)) return model_result(new_T, model, iter + 1, true, H, n_points);
    T = new_T;
    prev_error = model.error;
  }
  // (max_iterations <= 0: the initial guess with the statistics of an empty model — fitness 0, rmse +inf, no covariance)
  return model_result(T, last_model, crit.max_iterations > 0 ? crit.max_iterations : 0, false, last_H, n_points);
}

}  // namespace reg
}  // namespace fdm
