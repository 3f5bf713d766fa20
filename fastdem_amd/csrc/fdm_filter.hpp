// fdm_filter.hpp — the cloud filters on the device: nanopcl::filters::radiusOutlierRemoval, the crop family and
// removeInvalid.  gfx950.  Host side: fdm_engine_filter.inl; host algebra: fdm_filter_host.hpp.
//
// References being reproduced: filters/impl/outlier_removal_impl.hpp:21-77 over search/impl/voxel_hash_impl.hpp:13-64,
// :118-161; filters/impl/crop_impl.hpp; filters/core.hpp:95-109.  All fp32 arithmetic is written with the _rn
// intrinsics: no contraction.
//
// RADIUS OUTLIER REMOVAL.  The relation is clustering's (fdm_cluster.hpp, THE RELATION): count[i] = the number of j != i
// — by INDEX: a duplicate coordinate counts — whose voxels differ from i's by at most `range` on every axis and whose
// dist_sq = dx*dx + (dy*dy + dz*dz) <= r_sq; keep[i] = count[i] >= min_neighbors.  The front half is clustering's,
// launched as it is: k_cluster_voxels (voxels, flags, bounding box), k_cluster_keys, fdm_rsort, k_cluster_gather — the
// points in sorted order as float4, w = the list position; the voxels x - range .. x + range of one (y, z) row are ONE
// interval of the sorted array.
//
//   k_ror_candidates   per sorted point the lengths of the (2 range + 1)^2 intervals of its FULL neighbourhood, less
//                      itself, summed: the candidate tests, the work bound's measure (fdm_filter_host.hpp)
//   k_ror_count        one lane per sorted point; per row two bisections of the sorted keys, then a walk over the
//                      interval testing the gathered float4s, the point itself skipped by sorted position.  The point's
//                      OWN row comes first.  Mask mode (counts == nullptr) stops a lane as soon as count == min_neighbors:
//                      in a dense cloud a lane ends after a handful of loads and bisects two rows, and only real outliers
//                      pay for their whole neighbourhood.  Count mode walks everything and writes the exact count.  Results
//                      go to the list position held in w.  Integer atomics for the stats only.
//
// THE PREDICATE FILTERS.  k_filter_keep: one lane per point, the predicates written as the reference writes them,
// comparison by comparison and never as the negation of the other mode — that fixes what a NaN does.
#pragma once

#include "fdm_cluster.hpp"
#include "fdm_filter_host.hpp"

namespace fdm {

struct RorStat {
  unsigned long long candidates, tests;
  uint32_t kept;
};

inline __global__ void k_ror_stat_init(RorStat* __restrict__ st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->candidates = st->tests = 0ull;
    st->kept = 0u;
  }
}

// the (y, z) rows of a sorted point's full neighbourhood over the key layout of ClusterBox
struct RorRows {
  unsigned sh_z;
  long long vy, vz;
  unsigned long long x_lo, x_hi;
  int range, W;
  __device__ __forceinline__ RorRows(unsigned long long k, const ClusterBox& B) {
    sh_z = B.bits_x + B.bits_y;
    const long long vx = (long long)(k & ((1ull << B.bits_x) - 1ull));
    vy = (long long)((k >> B.bits_x) & ((1ull << B.bits_y) - 1ull));
    vz = (long long)(k >> sh_z);
    range = B.range;
    W = 2 * range + 1;
    x_lo = (unsigned long long)(vx - range > 0 ? vx - range : 0);
    x_hi = (unsigned long long)(vx + range < (long long)B.ext[0] ? vx + range : (long long)B.ext[0]);
  }
  // row u of W * W, the point's own row FIRST (u = 0), the others in (dz, dy) order: its interval [lo, hi) of sorted
  // positions; false for a row outside the box
  __device__ __forceinline__ bool interval(int u, const ClusterBox& B, const unsigned long long* __restrict__ keys,
                                           unsigned m, unsigned& lo, unsigned& hi) const {
    const int centre = (W * W) / 2;
    const int t = u == 0 ? centre : (u <= centre ? u - 1 : u);
    const long long zz = vz + (t / W - range), yy = vy + (t % W - range);
    if (zz < 0 || zz > (long long)B.ext[2] || yy < 0 || yy > (long long)B.ext[1]) return false;
    const unsigned long long base = ((unsigned long long)zz << sh_z) | ((unsigned long long)yy << B.bits_x);
    lo = cluster_lower_bound(keys, 0u, m, base | x_lo);
    hi = cluster_lower_bound(keys, lo, m, (base | x_hi) + 1ull);
    return true;
  }
};

inline __global__ __launch_bounds__(256) void k_ror_candidates(unsigned m, const unsigned long long* __restrict__ keys,
                                                               const ClusterBox B, RorStat* __restrict__ st) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  unsigned long long sum = 0ull;
  if (q < m) {
    const RorRows R(keys[q], B);
    for (int u = 0; u < R.W * R.W; ++u) {
      unsigned lo, hi;
      if (R.interval(u, B, keys, m, lo, hi)) sum += hi - lo;
    }
    sum -= 1ull;  // (its own row holds the point itself)
  }
  sum = wave_sum(sum);
  if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(&st->candidates, sum);
}

// min_neighbors: clamped to 2^32 - 1 by the host (a count is below m < 2^32 - 1).  counts == nullptr: mask mode.
inline __global__ __launch_bounds__(256) void k_ror_count(unsigned m, const unsigned long long* __restrict__ keys,
                                                          const ClusterBox B, const float4* __restrict__ pts, float r_sq,
                                                          uint32_t min_neighbors, uint8_t* __restrict__ keep,
                                                          uint32_t* __restrict__ counts, RorStat* __restrict__ st) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  unsigned long long tests = 0ull;
  bool kept = false;
  if (q < m) {
    const float4 me = pts[q];
    const uint32_t limit = counts ? 0xFFFFFFFFu : min_neighbors;  // (count mode never reaches it)
    uint32_t count = 0u;
    const RorRows R(keys[q], B);
    for (int u = 0; u < R.W * R.W && count < limit; ++u) {
      unsigned lo, hi;
      if (!R.interval(u, B, keys, m, lo, hi)) continue;
      for (unsigned c = lo; c < hi && count < limit; ++c) {
        if (c == q) continue;
        const float4 o = pts[c];
        const float dx = __fsub_rn(o.x, me.x), dy = __fsub_rn(o.y, me.y), dz = __fsub_rn(o.z, me.z);
        const float d = __fadd_rn(__fmul_rn(dx, dx), __fadd_rn(__fmul_rn(dy, dy), __fmul_rn(dz, dz)));
        ++tests;
        if (d <= r_sq) ++count;
      }
    }
    kept = count >= min_neighbors;
    const uint32_t w = __float_as_uint(me.w);
    keep[w] = kept ? 1 : 0;
    if (counts) counts[w] = count;
  }
  tests = wave_sum(tests);
  const unsigned long long kept_lanes = __ballot(kept);
  if ((threadIdx.x & 63u) == 0u) {
    if (tests) atomicAdd(&st->tests, tests);
    if (kept_lanes) atomicAdd(&st->kept, unsigned(__popcll(kept_lanes)));
  }
}

// ---- the predicate filters ----
__device__ __forceinline__ bool filter_keeps(const filter::KeepParams& P, float x, float y, float z) {
  using namespace filter;
  const bool inside = P.mode == kKeepInside;
  const float* const a = P.a;
  switch (P.kind) {
    case kKeepBox:  // crop_impl.hpp:20-34
      return inside ? (x >= a[0] && x <= a[3] && y >= a[1] && y <= a[4] && z >= a[2] && z <= a[5])
                    : (x < a[0] || x > a[3] || y < a[1] || y > a[4] || z < a[2] || z > a[5]);
    case kKeepRange: {  // :62-79; squaredNorm in the three-term order of DESIGN.md §6
      const float d2 = __fadd_rn(__fmul_rn(x, x), __fadd_rn(__fmul_rn(y, y), __fmul_rn(z, z)));
      return inside ? (d2 >= a[0] && d2 <= a[1]) : (d2 < a[0] || d2 > a[1]);
    }
    case kKeepX:
    case kKeepY:
    case kKeepZ: {  // :106-183
      const float v = P.kind == kKeepX ? x : (P.kind == kKeepY ? y : z);
      return inside ? (v >= a[0] && v <= a[1]) : (v < a[0] || v > a[1]);
    }
    case kKeepAngle: {  // :185-208
      const float c_min = __fsub_rn(__fmul_rn(a[0], y), __fmul_rn(a[1], x));
      const float c_max = __fsub_rn(__fmul_rn(a[2], y), __fmul_rn(a[3], x));
      const bool in_range = P.flag ? (c_min >= -kAngleEps && c_max <= kAngleEps) : (c_min >= -kAngleEps || c_max <= kAngleEps);
      return in_range == inside;
    }
    default:  // kKeepFinite: filters/core.hpp:95-109
      return isfinite(x) && isfinite(y) && isfinite(z);
  }
}

constexpr unsigned kFilterMaxBlocks = 1024u;  // blocks of 256; a longer cloud is read by the strided loop

inline __global__ __launch_bounds__(256) void k_filter_stat_init(unsigned long long* __restrict__ kept) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *kept = 0ull;
}

inline __global__ __launch_bounds__(256) void k_filter_keep(unsigned n, const float* __restrict__ x,
                                                            const float* __restrict__ y, const float* __restrict__ z,
                                                            const filter::KeepParams P, uint8_t* __restrict__ keep,
                                                            unsigned long long* __restrict__ n_kept) {
  unsigned mine = 0u;
  const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
#pragma unroll 2  // (left to itself the compiler unrolls by eight over every kind: 148 VGPRs, three waves a SIMD)
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
    const bool k = filter_keeps(P, x[i], y[i], z[i]);
    keep[i] = k ? 1 : 0;
    mine += k ? 1u : 0u;
  }
  const unsigned long long total = wave_sum((unsigned long long)mine);
  if ((threadIdx.x & 63u) == 0u && total) atomicAdd(n_kept, total);
}

}  // namespace fdm
