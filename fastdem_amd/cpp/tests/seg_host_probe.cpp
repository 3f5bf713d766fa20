// seg_host_probe.cpp — the host algebra of RANSAC plane segmentation (csrc/fdm_segment_host.hpp) as a stand-alone CPU
// program: no device, no library.  Reads an operation and its numbers (hexadecimal floats) from standard input and prints
// the result the same way.  tests/test_seg_restate.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and
// holds it to the NumPy restatement.
//   1 n count                       -> the sampled triplets of `count` iterations over a list of n entries [3 * count]
//   2 n max_iterations probability batch passes counts[passes] valid[passes]
//                                   -> iterations, best_count, best_iter, n_invalid of the loop replayed in batches
//                                      (passes the list does not hold are fed as zero counts of valid models)
//   3 ratio probability             -> computeAdaptiveIterations
//   4 c00 c01 c02 c11 c12 c22       -> the unit eigenvector of the smallest eigenvalue [3]
//   5 v[3] centroid[3] best[3]      -> the refined model [4]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fdm_segment_host.hpp"

int main() {
  std::vector<double> in;
  char tok[128];
  while (std::scanf("%127s", tok) == 1) in.push_back(std::strtod(tok, nullptr));
  if (in.empty()) return 2;
  const int op = int(in[0]);
  const double* a = in.data() + 1;
  const size_t n = in.size() - 1;
  std::vector<double> out;
  if (op == 1 && n == 2) {
    seg::XorShift64 rng(42);
    const uint64_t size = uint64_t(a[0]);
    for (int k = 0; k < int(a[1]); ++k) {
      uint32_t t[3];
      seg::draw_triplet(rng, size, t);
      for (uint32_t v : t) out.push_back(double(v));
    }
  } else if (op == 2 && n >= 5 && n == 5 + 2 * size_t(a[4])) {
    const int batch = int(a[3]), passes = int(a[4]);
    seg::Loop loop;
    loop.start(uint64_t(a[0]), int(a[1]), a[2]);
    if (batch < 1 || passes < 0) return 2;
    const size_t width = size_t(batch);
    std::vector<uint32_t> counts(width), valid(width);
    while (loop.running()) {
      const int nb = std::min(batch, loop.remaining());
      for (int j = 0; j < nb; ++j) {
        const int it = loop.iter + j;
        counts[size_t(j)] = it < passes ? uint32_t(a[5 + it]) : 0u;
        valid[size_t(j)] = it < passes ? uint32_t(a[5 + passes + it]) : 1u;
      }
      loop.replay(counts.data(), valid.data(), nb);
    }
    out = {double(loop.iter), double(loop.best_count), double(loop.best_iter), double(loop.n_invalid)};
  } else if (op == 3 && n == 2) {
    out.push_back(double(seg::adaptive_iterations(a[0], a[1])));
  } else if (op == 4 && n == 6) {
    double v[3];
    seg::smallest_eigenvector(a, v);
    out.assign(v, v + 3);
  } else if (op == 5 && n == 9) {
    const float best[3] = {float(a[6]), float(a[7]), float(a[8])};
    float m[4];
    seg::refined_model(a, a + 3, best, m);
    for (float v : m) out.push_back(double(v));
  } else {
    return 2;
  }
  for (double v : out) std::printf("%a\n", v);
  return 0;
}
