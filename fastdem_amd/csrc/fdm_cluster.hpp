// fdm_cluster.hpp — Euclidean clustering on the device: nanopcl::segmentation::euclideanCluster.  gfx950.  Host side:
// fdm_engine_cluster.inl.
//
// Reference being reproduced: lib/nanoPCL/include/nanopcl/segmentation/impl/euclidean_cluster_impl.hpp:89-186 over
// search/impl/voxel_hash_impl.hpp:118-161 and core/voxel.hpp:28-80.  All fp32 arithmetic is written with the _rn
// intrinsics: no contraction.
//
// THE RELATION.  inv = 1.0f / tol, range = int(ceil(tol * inv)), r_sq = tol * tol, all fp32.  A point's voxel is
// floor(c * inv) per axis — the fp32 PRODUCT with the reciprocal (voxel.hpp:29-31), not segmentGround's division.  Points
// i and j are neighbours iff their voxel coordinates differ by at most `range` on every axis (the voxels radius() visits)
// and dist_sq <= r_sq, dist_sq = dx*dx + (dy*dy + dz*dz) of the fp32 differences: the three-term order of DESIGN.md §6
// (sum3), FIXED here.  The clusters are the connected components of that relation over the listed points; a component is
// kept iff min_size <= size <= max_size.
//
// THE ORDER (this project's, the reference's under a stable sort).  Kept clusters in descending size, equal sizes by
// their smallest list position ascending; inside a cluster ascending list position.
//
//   k_seg_index_check   (fdm_segment.hpp) reads the list only: an entry >= n is refused before any kernel addresses with one
//   k_cluster_voxels    per list position: the voxel, biased by 2^20 as voxel::pack biases it; flags for a coordinate that
//                       is not finite (the reference casts NaN to int) and for a voxel outside [-2^20 + range, 2^20 - 1 -
//                       range] (the reference clamps: the table degenerates); the voxels' bounding box
//   k_cluster_keys      the key [z][y][x] of voxel::pack over the bounding box, so that the sort needs few passes
//   fdm_rsort           stable sort of (key, list position): a voxel is one run, its positions ascending
//   k_cluster_gather    the points in sorted order as float4, w = the list position
//   k_cluster_ranges    x is the minor field of the key: the voxels x - range .. x + range of one (y, z) row are ONE
//                       interval of the sorted array.  Every pair is tested once, by its member at the higher sorted
//                       position, so a point needs the rows (dz, dy) <= (0, 0) only — 5 of 9 for range 1, 13 of 25 for
//                       range 2 — its own row cut at itself: two bisections of at most 32 steps per row.  Sums the
//                       intervals' lengths: the candidate pairs, the work bound's measure (fdm_engine_cluster.inl)
//   k_cluster_merge     one lane per sorted point walks its intervals: the distance test (the candidate's float4 is
//                       loaded for its position anyway; the roots are a chain of dependent loads, so they are read on a
//                       hit only), then unite.  parent[] over list positions, parent[v] <= v at all times: find with path
//                       halving, unite by a compare-and-swap of the larger root's parent to the smaller root; after a
//                       lost swap the DISPLACED pair (what the root was linked to, the other root) is united instead, so
//                       no link is dropped.  No waits between blocks, no grid barrier, no locks; find gives up after m
//                       steps, unite after kClusterMaxRetries lost swaps, each with a bit in ClusterStat::err: the kernel
//                       ends whatever the input.  A lost swap means another lane linked that root in the few hundred
//                       nanoseconds between this lane's find and its swap, and the next root is strictly smaller.
//   k_cluster_flatten   root[p] = find(p): the component's smallest position by the invariant, which is the tie-break
//                       key; sizes per root with integer atomics; the components counted
//   k_cluster_flags     keep[p] = min_size <= size[root[p]] <= max_size; the kept components counted
//   k_dem_count / k_pack_scan / k_seg_compact   the kept positions, ascending
//   k_cluster_order_keys  key = (m - size) << bits(m - 1) | root; ONE stable sort of (key, position) whose input is in
//                       ascending position: clusters by descending size then root, the order inside a cluster for free
//   k_seg_head_count / k_pack_scan / k_seg_heads   run heads = offsets
//   k_cluster_emit      cluster_indices (the list's entries at the sorted positions) and labels (cluster number + 1)
#pragma once

#include "fdm_device.hpp"
#include "fdm_segment.hpp"
#include "fdm_cluster_host.hpp"

namespace fdm {

constexpr int kClusterOffset = 1 << 20;       // voxel::COORD_OFFSET
constexpr unsigned kClusterMaxRetries = 4096u;
constexpr uint32_t kClusterBadFinite = 1u, kClusterBadVoxel = 2u;
constexpr uint32_t kClusterErrFind = 1u, kClusterErrRetry = 2u;

struct ClusterStat {
  uint32_t bad;             // kClusterBad*
  uint32_t err;             // kClusterErr*
  uint32_t lo[3], hi[3];    // the biased voxels' bounding box
  uint32_t components, kept;
  unsigned long long pairs, hits, unions;
};

inline __global__ void k_cluster_stat_init(ClusterStat* __restrict__ st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->bad = st->err = 0u;
    for (int k = 0; k < 3; ++k) { st->lo[k] = 0xFFFFFFFFu; st->hi[k] = 0u; }
    st->components = st->kept = 0u;
    st->pairs = st->hits = st->unions = 0ull;
  }
}

// floor(c * inv) biased by 2^20; false outside [-2^20 + range, 2^20 - 1 - range] (both bounds are floats)
__device__ __forceinline__ bool cluster_voxel_of(float c, float inv, int range, uint32_t& biased) {
  const float f = floorf(__fmul_rn(c, inv));
  if (!(f >= float(-kClusterOffset + range)) || !(f <= float(kClusterOffset - 1 - range))) return false;
  biased = uint32_t(int(f) + kClusterOffset);
  return true;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

inline __global__ __launch_bounds__(256) void k_cluster_voxels(unsigned m, const uint32_t* __restrict__ indices,
                                                               const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ z, float inv, int range,
                                                               unsigned long long* __restrict__ vox,
                                                               ClusterStat* __restrict__ st) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  uint32_t bad = 0u;
  uint32_t u[3] = {0u, 0u, 0u};
  if (p < m) {
    const uint32_t i = indices ? indices[p] : p;
    const float c[3] = {x[i], y[i], z[i]};
    if (!isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2])) bad = kClusterBadFinite;
    else if (!cluster_voxel_of(c[0], inv, range, u[0]) || !cluster_voxel_of(c[1], inv, range, u[1]) ||
             !cluster_voxel_of(c[2], inv, range, u[2]))
      bad = kClusterBadVoxel;
    if (bad) u[0] = u[1] = u[2] = 0u;
    vox[p] = (static_cast<unsigned long long>(u[2]) << 42) | (static_cast<unsigned long long>(u[1]) << 21) | u[0];
  }
  const bool live = p < m && !bad;
  uint32_t lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = live ? u[k] : 0xFFFFFFFFu; hi[k] = live ? u[k] : 0u; }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = min(lo[k], uint32_t(__shfl_xor(int(lo[k]), s)));
      hi[k] = max(hi[k], uint32_t(__shfl_xor(int(hi[k]), s)));
    }
  uint32_t any = bad;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) any |= uint32_t(__shfl_xor(int(any), s));
  if ((threadIdx.x & 63u) == 0u) {
    if (any) atomicOr(&st->bad, any);
    if (lo[0] <= hi[0]) {  // (a plain look first, as in k_seg_cell_keys: the box only grows)
      const volatile ClusterStat* const seen = st;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (lo[k] < seen->lo[k]) atomicMin(&st->lo[k], lo[k]);
        if (hi[k] > seen->hi[k]) atomicMax(&st->hi[k], hi[k]);
      }
    }
  }
}

// ClusterBox (fdm_cluster_host.hpp): what the keys are packed with
inline __global__ __launch_bounds__(256) void k_cluster_keys(unsigned m, const unsigned long long* __restrict__ vox,
                                                             const ClusterBox B, unsigned long long* __restrict__ keys) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= m) return;
  const unsigned long long v = vox[p];
  const unsigned long long ux = uint32_t(v & 0x1FFFFFull) - B.lo[0], uy = uint32_t((v >> 21) & 0x1FFFFFull) - B.lo[1],
                           uz = uint32_t(v >> 42) - B.lo[2];
  keys[p] = (uz << (B.bits_x + B.bits_y)) | (uy << B.bits_x) | ux;
}

inline __global__ __launch_bounds__(256) void k_cluster_gather(unsigned m, const uint32_t* __restrict__ pos,
                                                               const uint32_t* __restrict__ indices,
                                                               const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ z, float4* __restrict__ pts) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= m) return;
  const uint32_t p = pos[q];
  const uint32_t i = indices ? indices[p] : p;
  pts[q] = make_float4(x[i], y[i], z[i], __uint_as_float(p));
}

// first position in [lo, hi) whose key is not below k; hi if there is none.  At most 32 steps: hi - lo < 2^32.
__device__ __forceinline__ unsigned cluster_lower_bound(const unsigned long long* __restrict__ keys, unsigned lo,
                                                        unsigned hi, unsigned long long k) {
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const unsigned mid = lo + (hi - lo) / 2u;
    if (keys[mid] < k) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

__host__ __device__ constexpr int cluster_rows(int range) { return ((2 * range + 1) * (2 * range + 1) + 1) / 2; }

// iv[(2 t) m + q], iv[(2 t + 1) m + q] = the interval [lo, hi) of sorted positions that row t of sorted point q holds
// below q; row t is (dz, dy) = (t / W - range, t % W - range), W = 2 range + 1, the last one (0, 0)
inline __global__ __launch_bounds__(256) void k_cluster_ranges(unsigned m, const unsigned long long* __restrict__ keys,
                                                               const ClusterBox B, uint32_t* __restrict__ iv,
                                                               ClusterStat* __restrict__ st) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  unsigned long long pairs = 0ull;
  if (q < m) {
    const unsigned long long k = keys[q];
    const unsigned sh_z = B.bits_x + B.bits_y;
    const long long vx = (long long)(k & ((1ull << B.bits_x) - 1ull));
    const long long vy = (long long)((k >> B.bits_x) & ((1ull << B.bits_y) - 1ull));
    const long long vz = (long long)(k >> sh_z);
    const int W = 2 * B.range + 1, rows = cluster_rows(B.range);
    const unsigned long long x_lo = (unsigned long long)(vx - B.range > 0 ? vx - B.range : 0);
    const unsigned long long x_hi = (unsigned long long)(vx + B.range < (long long)B.ext[0] ? vx + B.range : (long long)B.ext[0]);
    for (int t = 0; t < rows; ++t) {
      const long long zz = vz + (t / W - B.range), yy = vy + (t % W - B.range);
      unsigned lo = q, hi = q;
      if (zz >= 0 && zz <= (long long)B.ext[2] && yy >= 0 && yy <= (long long)B.ext[1]) {
        const unsigned long long base = ((unsigned long long)zz << sh_z) | ((unsigned long long)yy << B.bits_x);
        lo = cluster_lower_bound(keys, 0u, q, base | x_lo);
        hi = t == rows - 1 ? q : cluster_lower_bound(keys, lo, q, (base | x_hi) + 1ull);
      }
      iv[size_t(2 * t) * m + q] = lo;
      iv[size_t(2 * t + 1) * m + q] = hi;
      pairs += hi - lo;
    }
  }
  pairs = wave_sum(pairs);
  if ((threadIdx.x & 63u) == 0u && pairs) atomicAdd(&st->pairs, pairs);
}

// ---- the union-find: parent[] over list positions, parent[v] <= v at all times.  Every access is a relaxed atomic of
// agent scope: the words carry no other data, so nothing has to be published behind them ----
__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of v, with path halving (a position that is no root never becomes one again, and what is stored into its
// word is one of its ancestors: a stale store keeps the tree and the invariant); gives up after `limit` steps
__device__ __forceinline__ uint32_t uf_find(uint32_t* __restrict__ parent, uint32_t v, unsigned limit, uint32_t* err) {
  for (unsigned steps = 0; steps <= limit; ++steps) {
    const uint32_t p = uf_load(parent + v);
    if (p == v) return v;
    const uint32_t g = uf_load(parent + p);
    if (g == p) return p;
    __hip_atomic_store(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v = g;
  }
  *err |= kClusterErrFind;
  return v;
}
// true: this call made the link
__device__ __forceinline__ bool uf_unite(uint32_t* __restrict__ parent, uint32_t a, uint32_t b, unsigned limit,
                                         uint32_t* err) {
  for (unsigned tries = 0; tries <= kClusterMaxRetries; ++tries) {
    a = uf_find(parent, a, limit, err);
    b = uf_find(parent, b, limit, err);
    if (a == b || *err) return false;
    if (a < b) { const uint32_t t = a; a = b; b = t; }  // a: the larger root
    uint32_t expect = a;
    if (__hip_atomic_compare_exchange_strong(parent + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return true;
    a = expect;  // a was linked to `expect` < a meanwhile: the displaced pair (expect, b) is still to be united
  }
  *err |= kClusterErrRetry;
  return false;
}

inline __global__ __launch_bounds__(256) void k_cluster_init(unsigned m, uint32_t* __restrict__ parent,
                                                             uint32_t* __restrict__ size) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p < m) { parent[p] = p; size[p] = 0u; }
}

inline __global__ __launch_bounds__(256) void k_cluster_merge(unsigned m, const float4* __restrict__ pts,
                                                              const uint32_t* __restrict__ iv, int rows, float r_sq,
                                                              uint32_t* __restrict__ parent,
                                                              ClusterStat* __restrict__ st) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  unsigned long long hits = 0ull, unions = 0ull;
  uint32_t err = 0u;
  if (q < m) {
    const float4 me = pts[q];
    const uint32_t mine = __float_as_uint(me.w);
    for (int t = 0; t < rows && !err; ++t) {
      const unsigned lo = iv[size_t(2 * t) * m + q], hi = min(iv[size_t(2 * t + 1) * m + q], q);
      for (unsigned c = lo; c < hi && !err; ++c) {
        const float4 o = pts[c];
        const float dx = __fsub_rn(o.x, me.x), dy = __fsub_rn(o.y, me.y), dz = __fsub_rn(o.z, me.z);
        const float d = sum3(__fmul_rn(dx, dx), __fmul_rn(dy, dy), __fmul_rn(dz, dz));
        if (d <= r_sq) {
          ++hits;
          if (uf_unite(parent, mine, __float_as_uint(o.w), m, &err)) ++unions;
        }
      }
    }
  }
  hits = wave_sum(hits);
  unions = wave_sum(unions);
  const uint32_t any = uint32_t(__ballot(err & kClusterErrFind) ? kClusterErrFind : 0u) |
                       uint32_t(__ballot(err & kClusterErrRetry) ? kClusterErrRetry : 0u);
  if ((threadIdx.x & 63u) == 0u) {
    if (hits) atomicAdd(&st->hits, hits);
    if (unions) atomicAdd(&st->unions, unions);
    if (any) atomicOr(&st->err, any);
  }
}

// (the merge is over: the trees no longer change, a plain walk finds the root)
inline __global__ __launch_bounds__(256) void k_cluster_flatten(unsigned m, const uint32_t* __restrict__ parent,
                                                                uint32_t* __restrict__ root, uint32_t* __restrict__ size,
                                                                ClusterStat* __restrict__ st) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  bool is_root = false, lost = false;
  uint32_t mine = 0u;
  if (p < m) {
    uint32_t v = p;
    unsigned steps = 0;
    for (; steps <= m; ++steps) {
      const uint32_t up = parent[v];
      if (up == v) break;
      v = up;
    }
    lost = steps > m;
    root[p] = v;
    mine = v;
    is_root = v == p;
  }
  // the lanes of a wavefront that found the same root add to its size once (a component of a million points is a
  // million additions to one word otherwise: this stage took 13.9 ms on the 2.1 M-point bench cloud, 0.30 ms so); at
  // most 64 rounds
  const unsigned lane = threadIdx.x & 63u;
  for (unsigned long long todo = __ballot(p < m); todo;) {
    const int leader = __ffsll(todo) - 1;
    const uint32_t r = uint32_t(__shfl(int(mine), leader));
    const unsigned long long same = __ballot(p < m && mine == r) & todo;
    if (int(lane) == leader) atomicAdd(&size[r], unsigned(__popcll(same)));
    todo &= ~same;
  }
  const unsigned long long roots = __ballot(is_root), bad = __ballot(lost);
  if ((threadIdx.x & 63u) == 0u) {
    if (roots) atomicAdd(&st->components, unsigned(__popcll(roots)));
    if (bad) atomicOr(&st->err, kClusterErrFind);
  }
}

inline __global__ __launch_bounds__(256) void k_cluster_flags(unsigned m, const uint32_t* __restrict__ root,
                                                              const uint32_t* __restrict__ size,
                                                              unsigned long long min_size, unsigned long long max_size,
                                                              uint8_t* __restrict__ keep, ClusterStat* __restrict__ st) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  bool kept_root = false;
  if (p < m) {
    const uint32_t r = root[p];
    const unsigned long long s = size[r];
    const bool in = s >= min_size && s <= max_size;
    keep[p] = in ? 1 : 0;
    kept_root = in && r == p;
  }
  const unsigned long long heads = __ballot(kept_root);
  if ((threadIdx.x & 63u) == 0u && heads) atomicAdd(&st->kept, unsigned(__popcll(heads)));
}

inline __global__ __launch_bounds__(256) void k_cluster_order_keys(unsigned total, const uint32_t* __restrict__ kept_pos,
                                                                   const uint32_t* __restrict__ root,
                                                                   const uint32_t* __restrict__ size, unsigned m,
                                                                   unsigned bits_root,
                                                                   unsigned long long* __restrict__ keys) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  if (j >= total) return;
  const uint32_t r = root[kept_pos[j]];
  keys[j] = (static_cast<unsigned long long>(m - size[r]) << bits_root) | r;
}

// entry j of the ordered (key, position) pairs: its list entry to cluster_indices[j], its cluster's number + 1 to
// labels[position].  offsets: k_pack_scan over k_seg_head_count's counts.
inline __global__ __launch_bounds__(256) void k_cluster_emit(unsigned total, const unsigned long long* __restrict__ keys,
                                                             const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ pos,
                                                             const uint32_t* __restrict__ indices,
                                                             uint32_t* __restrict__ cluster_indices,
                                                             uint32_t* __restrict__ labels) {
  __shared__ unsigned s_w[4];
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  bool head;
  const unsigned run = seg_run_of(total, keys, offsets, j, &head, s_w);
  if (j >= total) return;
  const uint32_t p = pos[j];
  cluster_indices[j] = indices ? indices[p] : p;
  if (labels) labels[p] = run + 1u;
}

}  // namespace fdm
