// fdm_segment_host.hpp — the host algebra of RANSAC plane segmentation (nanoPCL segmentation/impl/ransac_plane_impl.hpp):
// the sampler, the adaptive iteration count, the replay of the reference's sequential loop over a batch of device-made
// counts, the symmetric 3 x 3 eigenproblem of the refinement and the sign rule of the refined normal.  Plain C++17, no
// HIP: fdm_engine_segment.inl uses it, and cpp/tests/seg_host_probe.cpp compiles it alone.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace seg {

// detail::XorShift64 (:29-48)
struct XorShift64 {
  uint64_t state;
  explicit XorShift64(uint64_t seed = 42) : state(seed ? seed : 1) {}
  uint64_t next() {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
  }
  uint64_t rand_index(uint64_t n) { return next() % n; }
};

// One iteration's sample (:265-273): three draws first, then the two loops; POSITIONS in the index list of n >= 3 entries.
// The draws never depend on whether the model of the sample is valid.
inline void draw_triplet(XorShift64& rng, uint64_t n, uint32_t out[3]) {
  uint64_t i1 = rng.rand_index(n);
  uint64_t i2 = rng.rand_index(n);
  uint64_t i3 = rng.rand_index(n);
  while (i2 == i1) i2 = rng.rand_index(n);
  while (i3 == i1 || i3 == i2) i3 = rng.rand_index(n);
  out[0] = uint32_t(i1);
  out[1] = uint32_t(i2);
  out[2] = uint32_t(i3);
}

// detail::computeAdaptiveIterations (:56-71)
inline int adaptive_iterations(double inlier_ratio, double probability) {
  if (inlier_ratio <= 0.0 || inlier_ratio >= 1.0) return std::numeric_limits<int>::max();
  const double w_cubed = inlier_ratio * inlier_ratio * inlier_ratio;
  const double log_prob = std::log(1.0 - probability);
  const double log_outlier = std::log(1.0 - w_cubed);
  if (log_outlier >= 0.0) return std::numeric_limits<int>::max();
  const double k = std::ceil(log_prob / log_outlier);
  // static_cast<int> of a value outside int is undefined in the reference: saturated here (a NaN: INT_MAX)
  if (!(k < 2147483647.0)) return std::numeric_limits<int>::max();
  if (k < -2147483648.0) return std::numeric_limits<int>::min();
  return int(k);
}

// The state of the loop of :253-305 between batches.
struct Loop {
  uint64_t n = 0;            // indices.size()
  int max_iterations = 0;
  double probability = 0.0;
  int adaptive = 0;          // adaptive_iterations, starts at max_iterations (:255)
  int iter = 0;              // the loop variable: passes made so far
  uint64_t best_count = 0;
  int best_iter = -1;        // the pass that set the best model, -1: none yet
  uint64_t n_invalid = 0;    // passes whose sample gave no valid model
  void start(uint64_t n_, int max_iterations_, double probability_) {
    *this = Loop{};
    n = n_;
    max_iterations = max_iterations_;
    probability = probability_;
    adaptive = max_iterations_;
  }
  bool running() const { return iter < max_iterations && iter < adaptive; }
  // passes the loop can still make as things stand: an upper bound for the next batch
  int remaining() const { return running() ? (adaptive < max_iterations ? adaptive : max_iterations) - iter : 0; }
  // The passes iter .. iter + nb - 1 in order, with the counts and validity bits of their models; stops at the exact pass
  // at which the sequential code stops.  Returns the position inside the batch of the last best-update, -1 for none:
  // counts past the stop influence nothing.
  int replay(const uint32_t* counts, const uint32_t* valid, int nb) {
    int updated = -1;
    for (int j = 0; j < nb && running(); ++j) {
      ++iter;
      if (!valid[j]) { ++n_invalid; continue; }                       // :283-285
      if (uint64_t(counts[j]) > best_count) {                         // :296
        best_count = counts[j];
        best_iter = iter - 1;
        updated = j;
        const double ratio = static_cast<double>(counts[j]) / double(n);  // :301
        adaptive = adaptive_iterations(ratio, probability);
      }
    }
    return updated;
  }
};

// ---- the refinement's eigenproblem (:168-179): cyclic Jacobi in double on the symmetric matrix
// [c00 c01 c02; c01 c11 c12; c02 c12 c22]; the unit eigenvector of the smallest eigenvalue ----
inline void smallest_eigenvector(const double c[6], double v[3]) {
  double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 64; ++sweep) {
    const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
    if (!(off > 0.0)) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < 3; ++k) {  // A <- A J
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = cs * akp - sn * akq;
          a[k][q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < 3; ++k) {  // A <- J^T A
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = cs * apk - sn * aqk;
          a[q][k] = sn * apk + cs * aqk;
        }
        a[p][q] = a[q][p] = 0.0;
        for (int k = 0; k < 3; ++k) {  // V <- V J
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
  }
  int m = 0;
  for (int k = 1; k < 3; ++k)
    if (a[k][k] < a[m][m]) m = k;
  const double len = std::sqrt(V[0][m] * V[0][m] + V[1][m] * V[1][m] + V[2][m] * V[2][m]);
  for (int k = 0; k < 3; ++k) v[k] = len > 0.0 ? V[k][m] / len : V[k][m];
}

// fp32 in the project's three-term order a0 + (a1 + a2); volatile keeps a host compiler from contracting
inline float sum3f(float a0, float a1, float a2) {
  volatile float inner = a1 + a2;
  volatile float outer = a0 + inner;
  return outer;
}
inline float mulf(float a, float b) {
  volatile float p = a * b;
  return p;
}

// The refined model (:179-187) from the eigenvector and the centroid: the vector cast to float and normalized in fp32,
// the sign rule, d = -(n . float(centroid)).  SIGN (this project's definition; Eigen's follows its QL iteration): the dot
// of the refined normal with the best sample model's normal, taken in double, is not negative; where it is exactly 0 the
// first non-zero component is positive.
inline void refined_model(const double v[3], const double centroid[3], const float best_normal[3], float out[4]) {
  float n[3] = {float(v[0]), float(v[1]), float(v[2])};
  const float sq = sum3f(mulf(n[0], n[0]), mulf(n[1], n[1]), mulf(n[2], n[2]));
  if (sq > 0.0f) {  // Eigen's normalize(): left alone at zero length
    const float norm = std::sqrt(sq);
    for (float& c : n) c = c / norm;
  }
  const double dot = double(n[0]) * double(best_normal[0]) + double(n[1]) * double(best_normal[1]) +
                     double(n[2]) * double(best_normal[2]);
  bool flip = dot < 0.0;
  if (dot == 0.0) {
    for (int k = 0; k < 3; ++k)
      if (n[k] != 0.0f) { flip = n[k] < 0.0f; break; }
  }
  if (flip)
    for (float& c : n) c = -c;
  const float cf[3] = {float(centroid[0]), float(centroid[1]), float(centroid[2])};
  out[0] = n[0];
  out[1] = n[1];
  out[2] = n[2];
  out[3] = -sum3f(mulf(n[0], cf[0]), mulf(n[1], cf[1]), mulf(n[2], cf[2]));
}

}  // namespace seg
