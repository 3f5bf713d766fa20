// fdm_filter_host.hpp — the host algebra of the cloud filters (kernels: fdm_filter.hpp, host side:
// fdm_engine_filter.inl): cropAngle's constants, cropRange's squares, the work bound of the radius outlier removal.
// Plain C++, no HIP: cpp/tests/filter_host_probe.cpp exercises it under the sanitizers.
#pragma once

#include <cmath>
#include <cstdint>

namespace fdm {
namespace filter {

// The work bound of fdm_cloud_radius_outlier_removal: candidate tests (the sum over the points of the lengths of their
// full-neighbourhood intervals, less the point itself) above which a call is refused.  The constant is clustering's
// cluster::kMaxPairs in value, but this stage's own: it is held against k_ror_count's measured rate, not k_cluster_merge's.
// RATE, measured on the MI355X in count mode, which walks everything (profiles/r20/filters/README.md): k_ror_count tests
// 0.83e12 - 1.02e12 candidates a second on the 272 K-point RGB-D frame (5.9e10 in 58 ms at radius 1.0) and 0.93e12 -
// 1.69e12 on the 2.1 M-point scan at radii 0.3 and 1.0 (2.6e11 at radius 0.1, where the kernel takes 1 ms and the
// bisections are its cost), 0.42e12 - 1.57e12 on one voxel of 65 536 - 262 144 points: the bound is 0.1 - 0.36 s of it,
// under the second it may allow, so it is not lowered.  The RGB-D frame at radius 1.0 is at 40 % of the bound.
constexpr uint64_t kMaxTests = 150000000000ull;

// cropAngle's constants exactly as filters/impl/crop_impl.hpp:188-195 computes them: fp32 throughout, cosf / sinf of the
// two angles, wrap = min > max, range = wrap ? 2.0f * float(M_PI) - (min - max) : max - min, use_and = range < float(M_PI)
struct AngleConstants {
  float cos_min, sin_min, cos_max, sin_max;
  float range;
  bool wrap, use_and;
};
inline AngleConstants angle_constants(float min_angle, float max_angle) {
  constexpr double kPi = 3.14159265358979323846;  // M_PI
  AngleConstants A;
  A.cos_min = std::cos(min_angle);
  A.sin_min = std::sin(min_angle);
  A.cos_max = std::cos(max_angle);
  A.sin_max = std::sin(max_angle);
  A.wrap = min_angle > max_angle;
  A.range = A.wrap ? (2.0f * static_cast<float>(kPi) - (min_angle - max_angle)) : (max_angle - min_angle);
  A.use_and = A.range < static_cast<float>(kPi);
  return A;
}
constexpr float kAngleEps = 1e-5f;

// what k_filter_keep reads: the predicate's kind and mode and its six floats
//   BOX            a[0..2] = min, a[3..5] = max
//   RANGE          a[0] = min * min, a[1] = max * max (fp32, crop_impl.hpp:66-67)
//   X, Y, Z        a[0] = min, a[1] = max
//   ANGLE          a[0..3] = cos_min, sin_min, cos_max, sin_max; flag = use_and
//   FINITE         none
struct KeepParams {
  int kind, mode, flag;
  float a[6];
};
constexpr int kKeepBox = 0, kKeepRange = 1, kKeepX = 2, kKeepY = 3, kKeepZ = 4, kKeepAngle = 5, kKeepFinite = 6;
constexpr int kKeepInside = 0, kKeepOutside = 1;

// false: a kind or a mode that does not exist
inline bool keep_params(int kind, int mode, const float lo[3], const float hi[3], KeepParams& P) {
  if (kind < kKeepBox || kind > kKeepFinite || (mode != kKeepInside && mode != kKeepOutside)) return false;
  P.kind = kind;
  P.mode = mode;
  P.flag = 0;
  for (int k = 0; k < 6; ++k) P.a[k] = 0.0f;
  if (kind == kKeepBox) {
    for (int k = 0; k < 3; ++k) { P.a[k] = lo[k]; P.a[3 + k] = hi[k]; }
  } else if (kind == kKeepRange) {
    P.a[0] = lo[0] * lo[0];
    P.a[1] = hi[0] * hi[0];
  } else if (kind == kKeepAngle) {
    const AngleConstants A = angle_constants(lo[0], hi[0]);
    P.a[0] = A.cos_min; P.a[1] = A.sin_min; P.a[2] = A.cos_max; P.a[3] = A.sin_max;
    P.flag = A.use_and ? 1 : 0;
  } else if (kind != kKeepFinite) {
    P.a[0] = lo[0];
    P.a[1] = hi[0];
  }
  return true;
}

}  // namespace filter
}  // namespace fdm
