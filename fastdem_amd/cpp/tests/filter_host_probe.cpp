// filter_host_probe.cpp — the host algebra of the cloud filters (csrc/fdm_filter_host.hpp) as a stand-alone CPU program:
// no device, no library.  Reads an operation and its numbers (hexadecimal floats) from standard input and prints the
// result the same way.  tests/test_filter_restate.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer.
//   0                               -> checks cropAngle's algebra against the table below: wrap, the span, use_and at
//                                      exactly pi and one ulp below, min == max; prints the number of rows, exit 1 on a miss
//   1 min max                       -> cos_min, sin_min, cos_max, sin_max, range, wrap, use_and
//   2 kind mode lo[3] hi[3]         -> ok, kind, mode, flag, a[6] of what k_filter_keep reads
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fdm_filter_host.hpp"

namespace {
struct Row {
  float min, max;
  bool wrap;
  float range;
  bool use_and;
};
// pi = 0x1.921fb6p+1f = float(M_PI); the spans are what fp32 gives for crop_impl.hpp:192-193, worked out by hand
const Row kTable[] = {
    {-0x1.921fb6p-1f, 0x1.921fb6p-1f, false, 0x1.921fb6p+0f, true},  // (-pi/4, pi/4): a quarter turn
    {3.0f, -3.0f, true, 0x1.21fb6p-2f, true},                        // wrapped through pi: 2 pi - 6
    {0.0f, 0x1.921fb6p+1f, false, 0x1.921fb6p+1f, false},            // exactly pi: `<` fails, OR
    {0.0f, 0x1.921fb4p+1f, false, 0x1.921fb4p+1f, true},             // one ulp below pi: AND
    {1.0f, 1.0f, false, 0.0f, true},                                 // min == max: a ray, not wrapped
    {-0x1.921fb6p+1f, 0x1.921fb6p+1f, false, 0x1.921fb6p+2f, false}, // the full turn
    {0x1.921fb6p+1f, -0x1.921fb6p+1f, true, 0.0f, true},             // wrapped full turn: the span cancels to 0
    {2.0f, -2.0f, true, 0x1.243f6cp+1f, true},                       // 2 pi - 4 < pi
    {1.0f, -1.0f, true, 0x1.121fb6p+2f, false},                      // 2 pi - 2 > pi
    {-1.0f, 2.5f, false, 3.5f, false},
};
}  // namespace

int main() {
  using namespace fdm;
  std::vector<double> in;
  char tok[128];
  while (std::scanf("%127s", tok) == 1) in.push_back(std::strtod(tok, nullptr));
  if (in.empty()) return 2;
  const int op = int(in[0]);
  const double* a = in.data() + 1;
  const size_t n = in.size() - 1;
  std::vector<double> out;
  if (op == 0 && n == 0) {
    int rows = 0;
    for (const Row& r : kTable) {
      const filter::AngleConstants A = filter::angle_constants(r.min, r.max);
      if (A.wrap != r.wrap || A.range != r.range || A.use_and != r.use_and) {
        std::fprintf(stderr, "row %d: wrap %d range %a use_and %d\n", rows, int(A.wrap), double(A.range), int(A.use_and));
        return 1;
      }
      // the constants are the angles' own cosine and sine, on the unit circle to fp32
      const double norm_min = double(A.cos_min) * A.cos_min + double(A.sin_min) * A.sin_min;
      const double norm_max = double(A.cos_max) * A.cos_max + double(A.sin_max) * A.sin_max;
      if (std::fabs(norm_min - 1.0) > 1e-6 || std::fabs(norm_max - 1.0) > 1e-6) return 1;
      if (A.cos_min != std::cos(r.min) || A.sin_max != std::sin(r.max)) return 1;
      ++rows;
    }
    out = {double(rows)};
  } else if (op == 1 && n == 2) {
    const filter::AngleConstants A = filter::angle_constants(float(a[0]), float(a[1]));
    out = {double(A.cos_min), double(A.sin_min), double(A.cos_max), double(A.sin_max), double(A.range),
           A.wrap ? 1.0 : 0.0, A.use_and ? 1.0 : 0.0};
  } else if (op == 2 && n == 8) {
    const float lo[3] = {float(a[2]), float(a[3]), float(a[4])}, hi[3] = {float(a[5]), float(a[6]), float(a[7])};
    filter::KeepParams P{};
    const bool ok = filter::keep_params(int(a[0]), int(a[1]), lo, hi, P);
    out = {ok ? 1.0 : 0.0};
    if (ok) {
      out.insert(out.end(), {double(P.kind), double(P.mode), double(P.flag)});
      for (float v : P.a) out.push_back(double(v));
    }
  } else {
    return 2;
  }
  for (double v : out) std::printf("%a\n", v);
  return 0;
}
