// nanopcl/registration/vgicp_lookup.hpp — the host side of a voxel distribution map's lookup: voxel::pack of the reference
// (lib/nanoPCL/include/nanopcl/core/voxel.hpp:28-42) and a binary search over the map's keys, which the engine hands out
// in ascending order (include/fdm_engine.h, fdm_voxel_map_records).  No dependency beyond the standard library, so that
// it can be built and run stand-alone under sanitizers (tests/vgicp_host_probe.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace nanopcl {
namespace registration {
namespace detail {

// float -> int32 as the reference's x86 build converts it (cvttss2si): INT_MIN outside the int range, NaN included.  The
// cast itself is undefined there in C++, hence the test first.
inline int32_t vgicp_cvt(float v) {
  if (!(v >= -2147483648.0f && v < 2147483648.0f)) return std::numeric_limits<int32_t>::min();
  return static_cast<int32_t>(v);
}

// voxel::pack: floor(v * inv) per axis, clamped to [-2^20, 2^20 - 1], [z:21][y:21][x:21]
inline uint64_t vgicp_pack(float x, float y, float z, float inv) {
  constexpr int32_t kOff = 1 << 20, kMin = -kOff, kMax = kOff - 1;
  int32_t i[3] = {vgicp_cvt(std::floor(x * inv)), vgicp_cvt(std::floor(y * inv)), vgicp_cvt(std::floor(z * inv))};
  for (int32_t& v : i) v = v < kMin ? kMin : (v > kMax ? kMax : v);
  return (uint64_t(i[2] + kOff) << 42) | (uint64_t(i[1] + kOff) << 21) | uint64_t(i[0] + kOff);
}

// the position of `key` among n ascending keys, or n
inline size_t vgicp_find(const uint64_t* keys, size_t n, uint64_t key) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && keys[lo] == key) ? lo : n;
}

}  // namespace detail
}  // namespace registration
}  // namespace nanopcl
