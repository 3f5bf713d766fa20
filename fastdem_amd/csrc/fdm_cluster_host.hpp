// fdm_cluster_host.hpp — the host algebra of Euclidean clustering (kernels: fdm_cluster.hpp, host side:
// fdm_engine_cluster.inl): the relation's constants, the key layout over the voxels' bounding box, the ordering key's
// widths, the work bound.  Plain C++, no HIP: cpp/tests/cluster_host_probe.cpp exercises it under the sanitizers.
#pragma once

#include <cmath>
#include <cstdint>

namespace fdm {

// what the keys are packed with: the bounding box's low corner (biased voxels), its extent, the fields' widths
struct ClusterBox {
  uint32_t lo[3], ext[3];  // ext = hi - lo
  unsigned bits_x, bits_y;
  int range;
};

namespace cluster {

constexpr int kMaxRange = 2;  // (2 range + 1)^2 rows are walked; the reference gives 1 for every tolerance tried
// The work bound: candidate pairs (the sum over the points of the lengths of their intervals) above which a call is
// refused.  Measured on the MI355X (profiles/r13/cluster/README.md): k_cluster_merge walks 1.36e11 candidate pairs a
// second on the 272 K-point RGB-D frame (1.6e10 in 120 ms) and 2.45e11 on one voxel of 524 288 points (1.37e11 in 560 ms):
// the bound is 0.6 - 1.1 s of it.  The RGB-D frame is at a tenth of the bound, the 2.1 M-point scan has 7.6e8, the
// largest test 1.25e7.
constexpr uint64_t kMaxPairs = 150000000000ull;

inline unsigned bits_of(uint64_t max_value) {  // bits a value of 0 .. max_value needs, at least one
  unsigned bits = 1;
  while (bits < 64u && (max_value >> bits) != 0u) ++bits;
  return bits;
}

struct Relation {
  float inv, r_sq;
  int range;
};
// VoxelHash(tol): inv = 1.0f / tol (voxel_hash.hpp:25); radius(): r_sq = r * r, range = int(ceil(r * inv))
// (voxel_hash_impl.hpp:122-123).  false: a tolerance that is not a positive finite number, or one whose range is not
// 1 .. kMaxRange (a reciprocal that overflowed)
inline bool relation(float tol, Relation& R) {
  if (!(tol > 0.0f) || !std::isfinite(tol)) return false;
  R.inv = 1.0f / tol;
  R.r_sq = tol * tol;
  const float c = std::ceil(tol * R.inv);
  if (!(c >= 1.0f) || !(c <= float(kMaxRange))) return false;
  R.range = int(c);
  return true;
}

// the key [z][y][x] over the box lo .. hi of biased voxels; false for an empty box.  Every field has at most 21 bits.
inline bool box(const uint32_t lo[3], const uint32_t hi[3], int range, ClusterBox& B, unsigned& bits) {
  for (int k = 0; k < 3; ++k) {
    if (lo[k] > hi[k] || hi[k] >= (1u << 21)) return false;
    B.lo[k] = lo[k];
    B.ext[k] = hi[k] - lo[k];
  }
  B.bits_x = bits_of(B.ext[0]);
  B.bits_y = bits_of(B.ext[1]);
  B.range = range;
  bits = B.bits_x + B.bits_y + bits_of(B.ext[2]);
  return true;
}

// the ordering key (m - size) << bits_root | root of m >= 1 list positions: m - size and root are both at most m - 1
inline void order_bits(uint32_t m, unsigned& bits_root, unsigned& bits) {
  bits_root = bits_of(uint64_t(m) - 1u);
  bits = 2u * bits_root;
}

}  // namespace cluster
}  // namespace fdm
