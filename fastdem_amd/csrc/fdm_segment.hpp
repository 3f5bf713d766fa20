// fdm_segment.hpp — cloud segmentation on the device: nanopcl::segmentation::segmentGround and segmentPlane /
// segmentMultiplePlanes (RANSAC).  gfx950.  Host side: fdm_engine_segment.inl; the host algebra: fdm_segment_host.hpp.
//
// Reference being reproduced: lib/nanoPCL/include/nanopcl/segmentation/impl/ground_seg_impl.hpp:27-123 and
// impl/ransac_plane_impl.hpp:29-405.  All fp32 arithmetic is written with the _rn intrinsics: no contraction.
//
// segmentGround
//   k_seg_cell_keys  per point: gx = int(floor(x / r)), gy likewise (a correctly rounded DIVISION, :33-34), the key
//                    [gy:32][gx:32] biased to unsigned, ord(z); a flag for a coordinate that is not finite or a floor
//                    outside int32, and the bounding box of the cells
//   fdm_rsort        stable sort of (ord(z), index), then — k_seg_pack_keys gathers the cells' keys, packed over the
//                    bounding box — stable sort by cell: every cell is one run, its z ascending (the two-sort device of
//                    fdm_dem.hpp)
//   k_seg_head_count / k_pack_scan / k_seg_heads    run heads by count-scan-write: pos[r] = first entry of run r
//   k_seg_cell_cut   per run: robust = z_sorted[min(size_t(percentile * float(count - 1)), count - 1)] (:54-57); the
//                    bits of robust + thickness, or -inf for an obstacle-only cell (:46-48, :60-62)
//   k_seg_classify   every sorted entry finds its run and writes is_ground / is_obstacle of its point (:100-102)
//   k_dem_count / k_pack_scan / k_seg_compact   the two index lists in input order
// segmentPlane
//   k_seg_index_check  reads the index list only: an entry >= n raises a flag before any kernel addresses with one
//   k_plane_models   one lane per hypothesis: PlaneModel::fromPoints (:196-215) of the sampled triplet
//   k_plane_count    the hot path: every hypothesis of the batch against every listed point in one pass over the cloud
//   k_plane_flags    collectInliers (:102-121) as a flag per list position; k_seg_compact writes the list
//   k_plane_sum      the refinement's sums in double (:142-166): a fixed grid, a fixed tree, no floating-point atomics
#pragma once

#include "fdm_device.hpp"

namespace fdm {

struct SegStat {
  uint32_t bad;        // ground: a coordinate that is not finite, or a floor outside int32; plane: an index >= n
  uint32_t min_x, max_x, min_y, max_y;  // biased cell coordinates
  uint32_t pad[3];
};

inline __global__ void k_seg_stat_init(SegStat* __restrict__ st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->bad = 0u;
    st->min_x = st->min_y = 0xFFFFFFFFu;
    st->max_x = st->max_y = 0u;
  }
}

// int(floor(v / r)) biased to unsigned; false where the reference's static_cast<int> is undefined
__device__ __forceinline__ bool seg_cell_of(float v, float r, uint32_t& biased) {
  const float f = floorf(__fdiv_rn(v, r));
  if (!(f >= -2147483648.0f) || !(f < 2147483648.0f)) return false;
  biased = uint32_t(int(f)) ^ 0x80000000u;
  return true;
}

inline __global__ __launch_bounds__(256) void k_seg_cell_keys(unsigned n, const float* __restrict__ x,
                                                              const float* __restrict__ y, const float* __restrict__ z,
                                                              float resolution, unsigned long long* __restrict__ cell,
                                                              uint32_t* __restrict__ zkey, SegStat* __restrict__ st) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  uint32_t gx = 0u, gy = 0u;
  if (i < n) {
    const float px = x[i], py = y[i], pz = z[i];
    bad = !isfinite(px) || !isfinite(py) || !isfinite(pz);
    if (!bad) bad = !seg_cell_of(px, resolution, gx) || !seg_cell_of(py, resolution, gy);
    if (bad) gx = gy = 0u;
    cell[i] = (static_cast<unsigned long long>(gy) << 32) | gx;
    zkey[i] = ord(pz);
  }
  const bool live = i < n && !bad;
  uint32_t lo_x = live ? gx : 0xFFFFFFFFu, hi_x = live ? gx : 0u, lo_y = live ? gy : 0xFFFFFFFFu, hi_y = live ? gy : 0u;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    lo_x = min(lo_x, uint32_t(__shfl_xor(int(lo_x), s)));
    hi_x = max(hi_x, uint32_t(__shfl_xor(int(hi_x), s)));
    lo_y = min(lo_y, uint32_t(__shfl_xor(int(lo_y), s)));
    hi_y = max(hi_y, uint32_t(__shfl_xor(int(hi_y), s)));
  }
  const unsigned long long mb = __ballot(bad);
  if ((threadIdx.x & 63u) == 0u) {
    if (mb) atomicOr(&st->bad, 1u);
    if (lo_x <= hi_x) {
      // (a plain look first: the box only grows, so a stale value can cost a needless atomic, never a missed one —
      // without it 32 K wavefronts of a 2.1 M-point cloud queue on four words: 1.5 ms for this kernel)
      const volatile SegStat* const seen = st;
      if (lo_x < seen->min_x) atomicMin(&st->min_x, lo_x);
      if (hi_x > seen->max_x) atomicMax(&st->max_x, hi_x);
      if (lo_y < seen->min_y) atomicMin(&st->min_y, lo_y);
      if (hi_y > seen->max_y) atomicMax(&st->max_y, hi_y);
    }
  }
}

// the second sort's keys: entry q of the z-sorted pairs gets its point's cell, packed over the bounding box
inline __global__ __launch_bounds__(256) void k_seg_pack_keys(unsigned n, const uint32_t* __restrict__ idx,
                                                              const unsigned long long* __restrict__ cell,
                                                              uint32_t min_x, uint32_t min_y, unsigned bits_x,
                                                              unsigned long long* __restrict__ keys) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= n) return;
  const unsigned long long c = cell[idx[q]];
  const unsigned long long gx = uint32_t(c) - min_x, gy = uint32_t(c >> 32) - min_y;
  keys[q] = (gy << bits_x) | gx;  // (bits_x <= 32)
}

// ---- run heads of the sorted keys, count-scan-write ----
inline __global__ __launch_bounds__(256) void k_seg_head_count(unsigned n, const unsigned long long* __restrict__ keys,
                                                               uint32_t* __restrict__ counts) {
  __shared__ unsigned s_w[4];
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  const bool head = p < n && (p == 0u || keys[p - 1u] != keys[p]);
  const unsigned long long m = __ballot(head);
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = unsigned(__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0u) counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// the run entry p belongs to: heads of earlier blocks + heads of this block at or before p, less one.  All 256 threads
// of the block call it (it holds a barrier).
__device__ __forceinline__ unsigned seg_run_of(unsigned n, const unsigned long long* __restrict__ keys,
                                               const uint32_t* __restrict__ offsets, unsigned p, bool* is_head,
                                               unsigned* s_w) {
  const bool head = p < n && (p == 0u || keys[p - 1u] != keys[p]);
  const unsigned long long m = __ballot(head);
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0u) s_w[w] = unsigned(__popcll(m));
  __syncthreads();
  unsigned upto = unsigned(__popcll(m & ((2ull << lane) - 1ull)));  // heads in lanes 0 .. lane
  for (unsigned q = 0; q < w; ++q) upto += s_w[q];
  *is_head = head;
  return offsets[blockIdx.x] + upto - 1u;  // (p < n: entry 0 is a head, so upto >= 1 from there on)
}

// pos[r] = first entry of run r; pos[n_runs] = n
inline __global__ __launch_bounds__(256) void k_seg_heads(unsigned n, const unsigned long long* __restrict__ keys,
                                                          const uint32_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ pos) {
  __shared__ unsigned s_w[4];
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  bool head;
  const unsigned r = seg_run_of(n, keys, offsets, p, &head, s_w);
  if (head) pos[r] = p;
  if (p == n - 1u) pos[offsets[gridDim.x]] = n;
}

struct GroundParams {
  float percentile, thickness, max_height;
  unsigned long long min_points;
};
constexpr uint32_t kSegAllObstacle = 0xFF800000u;  // -inf: every finite z is above it

// cut[r]: the bits of robust + thickness of run r, or kSegAllObstacle.  idx: the sorted pairs' point indices.
inline __global__ __launch_bounds__(256) void k_seg_cell_cut(unsigned n, const uint32_t* __restrict__ offsets,
                                                             unsigned blocks, const uint32_t* __restrict__ pos,
                                                             const uint32_t* __restrict__ idx,
                                                             const float* __restrict__ z, const GroundParams G,
                                                             uint32_t* __restrict__ cut) {
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  if (r >= offsets[blocks] || r >= n) return;
  const unsigned first = pos[r], count = pos[r + 1u] - first;
  uint32_t c = kSegAllObstacle;
  if (static_cast<unsigned long long>(count) >= G.min_points) {  // :46
    // :54-56: a float product, truncated; min() with count - 1 (which a product no uint32 holds, or no number, gets too)
    const float prod = __fmul_rn(G.percentile, __uint2float_rn(count - 1u));
    const unsigned k = prod < 4294967296.0f ? min(unsigned(prod), count - 1u) : count - 1u;
    const float robust = z[idx[first + k]];
    if (!(robust > G.max_height)) c = __float_as_uint(__fadd_rn(robust, G.thickness));  // :60, :102
  }
  cut[r] = c;
}

inline __global__ __launch_bounds__(256) void k_seg_classify(unsigned n, const unsigned long long* __restrict__ keys,
                                                             const uint32_t* __restrict__ idx,
                                                             const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ cut,
                                                             const float* __restrict__ z, uint8_t* __restrict__ is_ground,
                                                             uint8_t* __restrict__ is_obstacle) {
  __shared__ unsigned s_w[4];
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  bool head;
  const unsigned r = seg_run_of(n, keys, offsets, p, &head, s_w);
  if (p >= n) return;
  const uint32_t i = idx[p];
  const bool obstacle = z[i] > __uint_as_float(cut[r]);  // :100-102, strict
  is_ground[i] = obstacle ? 0 : 1;
  is_obstacle[i] = obstacle ? 1 : 0;
}

// ---- order-keeping compaction of a list: the kept positions' entries (src NULL: the positions themselves) move to
// offsets[block] + rank; counts: k_dem_count, offsets: k_pack_scan over them ----
inline __global__ __launch_bounds__(256) void k_seg_compact(unsigned n, const uint8_t* __restrict__ keep,
                                                            const uint32_t* __restrict__ offsets,
                                                            const uint32_t* __restrict__ src, uint32_t* __restrict__ out) {
  __shared__ unsigned s_w[4];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const bool in = i < n && keep[i] != 0;
  const unsigned long long m = __ballot(in);
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0u) s_w[w] = unsigned(__popcll(m));
  __syncthreads();
  if (!in) return;
  unsigned rank = unsigned(__popcll(m & ((1ull << lane) - 1ull)));
  for (unsigned q = 0; q < w; ++q) rank += s_w[q];
  out[size_t(offsets[blockIdx.x]) + rank] = src ? src[i] : i;
}
// keep[i] != 0 inverted into out[i] (the strike-out of segmentMultiplePlanes keeps what the plane did not take)
inline __global__ __launch_bounds__(256) void k_seg_invert(unsigned n, const uint8_t* __restrict__ keep,
                                                           uint8_t* __restrict__ out) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = keep[i] ? 0 : 1;
}

// ---- RANSAC ----
inline __global__ __launch_bounds__(256) void k_seg_index_check(unsigned m, const uint32_t* __restrict__ indices,
                                                                unsigned n, SegStat* __restrict__ st) {
  bool bad = false;
  for (unsigned long long p = blockIdx.x * 256u + threadIdx.x; p < m; p += gridDim.x * 256u) bad |= indices[p] >= n;
  if (__ballot(bad) && (threadIdx.x & 63u) == 0u) atomicOr(&st->bad, 1u);
}

// PlaneModel::fromPoints (:196-215), the arithmetic stated once: differences, the cross product as Eigen writes it, the
// norm in the three-term order, the quotient, d = -(n . p1).  false: collinear (norm < 1e-10f) or d not finite (isValid).
__device__ __forceinline__ bool plane_from_points(const float p1[3], const float p2[3], const float p3[3], float4& model) {
  const float ax = __fsub_rn(p2[0], p1[0]), ay = __fsub_rn(p2[1], p1[1]), az = __fsub_rn(p2[2], p1[2]);
  const float bx = __fsub_rn(p3[0], p1[0]), by = __fsub_rn(p3[1], p1[1]), bz = __fsub_rn(p3[2], p1[2]);
  float n0 = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
  float n1 = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
  float n2 = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
  // (sqrtf: correctly rounded under -fhip-fp32-correctly-rounded-divide-sqrt; __fsqrt_rn is the approximate root here)
  const float norm = sqrtf(sum3(__fmul_rn(n0, n0), __fmul_rn(n1, n1), __fmul_rn(n2, n2)));
  if (norm < 1e-10f) {
    model = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7FC00000u));
    return false;
  }
  n0 = __fdiv_rn(n0, norm); n1 = __fdiv_rn(n1, norm); n2 = __fdiv_rn(n2, norm);
  const float d = -sum3(__fmul_rn(n0, p1[0]), __fmul_rn(n1, p1[1]), __fmul_rn(n2, p1[2]));
  model = make_float4(n0, n1, n2, d);
  return isfinite(d);
}
// |n . p + d| of :91 / :114, the scalar expression left to right
__device__ __forceinline__ float plane_dist(const float4 m, float px, float py, float pz) {
  return fabsf(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m.x, px), __fmul_rn(m.y, py)), __fmul_rn(m.z, pz)), m.w));
}

// What a batch of hypotheses leaves for the host, read back in one copy: models, counts, validity bits.
constexpr int kSegMaxBatch = 128;
struct PlaneBatch {
  float4 model[kSegMaxBatch];
  uint32_t count[kSegMaxBatch];
  uint32_t valid[kSegMaxBatch];
};

// trip: 3 x nb positions in the index list (indices NULL: the points in order); also clears the batch's counts
inline __global__ __launch_bounds__(kSegMaxBatch) void k_plane_models(int nb, const uint32_t* __restrict__ trip,
                                                                       const uint32_t* __restrict__ indices,
                                                                       const float* __restrict__ x,
                                                                       const float* __restrict__ y,
                                                                       const float* __restrict__ z,
                                                                       PlaneBatch* __restrict__ B) {
  const int j = threadIdx.x;
  if (j >= nb) return;
  float p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t pos = trip[3 * j + k];
    const uint32_t i = indices ? indices[pos] : pos;
    p[k][0] = x[i]; p[k][1] = y[i]; p[k][2] = z[i];
  }
  float4 m;
  const bool ok = plane_from_points(p[0], p[1], p[2], m);
  B->model[j] = m;
  B->valid[j] = ok ? 1u : 0u;
  B->count[j] = 0u;
}

// The hot path: the nb <= kSegMaxBatch hypotheses of a batch against the m listed points in one pass.  A block walks
// tiles of 1 024 list positions, grid-stride; a lane holds four points of the tile in registers (coalesced loads, a
// gather where there is an index list) and the block's models sit in LDS, read at a wave-uniform address (a broadcast).
// Per hypothesis the four comparisons become four ballots, their population counts a wave-uniform sum, and lane j of the
// wavefront keeps the running count of hypotheses j and j + 64: two registers, no atomic and no LDS traffic per point.
// At the end the four wavefronts meet in LDS and the block adds at most one integer per hypothesis to global memory: the
// counts are exact and the same in every run.  An invalid model has a d that is not finite, a lane without a point has
// NaN coordinates: no such distance is below the threshold.
constexpr unsigned kSegTile = 1024u;
inline __global__ __launch_bounds__(256) void k_plane_count(unsigned m, const uint32_t* __restrict__ indices,
                                                            const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, float threshold, int nb,
                                                            PlaneBatch* __restrict__ B) {
  __shared__ float4 s_model[kSegMaxBatch];
  __shared__ uint32_t s_cnt[4][kSegMaxBatch];
  if (int(threadIdx.x) < nb) s_model[threadIdx.x] = B->model[threadIdx.x];
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const float nanv = __uint_as_float(0x7FC00000u);
  uint32_t cnt_lo = 0u, cnt_hi = 0u;
  const int nb_lo = min(nb, 64);
  for (unsigned long long base = blockIdx.x * kSegTile; base < m; base += gridDim.x * kSegTile) {
    float px[4], py[4], pz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned long long p = base + unsigned(r) * 256u + threadIdx.x;  // (64 bits: the last stride passes 2^32)
      px[r] = py[r] = pz[r] = nanv;
      if (p < m) {
        const uint32_t i = indices ? indices[p] : p;
        px[r] = x[i]; py[r] = y[i]; pz[r] = z[i];
      }
    }
    for (int j =0; j < nb_lo; ++j) {
      const float4 mj = s_model[j];
      unsigned c = 0u;
#pragma unroll
      for (int r = 0; r < 4; ++r) c += unsigned(__popcll(__ballot(plane_dist(mj, px[r], py[r], pz[r]) < threshold)));
      cnt_lo += lane == unsigned(j) ? c : 0u;
    }
    for (int j =64; j < nb; ++j) {
      const float4 mj = s_model[j];
      unsigned c = 0u;
#pragma unroll
      for (int r = 0; r < 4; ++r) c += unsigned(__popcll(__ballot(plane_dist(mj, px[r], py[r], pz[r]) < threshold)));
      cnt_hi += lane == unsigned(j - 64) ? c : 0u;
    }
  }
  s_cnt[w][lane] = cnt_lo;
  s_cnt[w][64u + lane] = cnt_hi;
  __syncthreads();
  if (int(threadIdx.x) < nb) {
    const uint32_t c = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
    if (c) atomicAdd(&B->count[threadIdx.x], c);
  }
}

// keep[p] = the listed point at position p is an inlier of `model` (:112-118)
inline __global__ __launch_bounds__(256) void k_plane_flags(unsigned m, const uint32_t* __restrict__ indices,
                                                            const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, float4 model, float threshold,
                                                            uint8_t* __restrict__ keep) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= m) return;
  const uint32_t i = indices ? indices[p] : p;
  keep[p] = plane_dist(model, x[i], y[i], z[i]) < threshold ? 1 : 0;
}

// ---- the refinement's sums (:142-166) in double.  MOMENTS false: the three coordinate sums; true: the six central
// second moments about c (c00 c01 c02 c11 c12 c22).  A fixed tree: lane t of block b sums entries b * 256 + t + k * grid *
// 256 in order of k, the block's 256 lanes meet in a binary tree in LDS, k_plane_sum_final meets the blocks' partials
// in the same tree.  The grid is a function of the inlier count alone (seg_sum_blocks): the sums are too. ----
constexpr unsigned kSegSumBlocks = 256u;
__host__ __device__ constexpr unsigned seg_sum_blocks(unsigned count) {
  return count == 0u ? 1u : ((count + 255u) / 256u < kSegSumBlocks ? (count + 255u) / 256u : kSegSumBlocks);
}
template <int W>
__device__ __forceinline__ void seg_block_tree(double (*s)[256], double v[W], double* out) {
  const unsigned t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < W; ++q) s[q][t] = v[q];
  __syncthreads();
  for (unsigned half = 128u; half > 0u; half >>= 1) {
    if (t < half)
#pragma unroll
      for (int q = 0; q < W; ++q) s[q][t] += s[q][t + half];
    __syncthreads();
  }
  if (t < unsigned(W)) out[t] = s[t][0];
}
template <bool MOMENTS>
__global__ __launch_bounds__(256) void k_plane_sum(unsigned count, const uint32_t* __restrict__ inliers,
                                                   const float* __restrict__ x, const float* __restrict__ y,
                                                   const float* __restrict__ z, double cx, double cy, double cz,
                                                   double* __restrict__ partial) {
  constexpr int W = MOMENTS ? 6 : 3;
  __shared__ double s[W][256];
  double v[W];
#pragma unroll
  for (int q = 0; q < W; ++q) v[q] = 0.0;
  for (unsigned long long p = blockIdx.x * 256u + threadIdx.x; p < count; p += gridDim.x * 256u) {
    const uint32_t i = inliers[p];
    if constexpr (MOMENTS) {
      const double dx = __dsub_rn(double(x[i]), cx), dy = __dsub_rn(double(y[i]), cy), dz = __dsub_rn(double(z[i]), cz);
      v[0] = __dadd_rn(v[0], __dmul_rn(dx, dx)); v[1] = __dadd_rn(v[1], __dmul_rn(dx, dy));
      v[2] = __dadd_rn(v[2], __dmul_rn(dx, dz)); v[3] = __dadd_rn(v[3], __dmul_rn(dy, dy));
      v[4] = __dadd_rn(v[4], __dmul_rn(dy, dz)); v[5] = __dadd_rn(v[5], __dmul_rn(dz, dz));
    } else {
      v[0] = __dadd_rn(v[0], double(x[i])); v[1] = __dadd_rn(v[1], double(y[i])); v[2] = __dadd_rn(v[2], double(z[i]));
    }
  }
  seg_block_tree<W>(s, v, partial + size_t(blockIdx.x) * W);
}
// out[0 .. W) = the tree over the `blocks` partials (one block of 256 lanes; lanes past `blocks` hold zeros)
template <int W>
__global__ __launch_bounds__(256) void k_plane_sum_final(unsigned blocks, const double* __restrict__ partial,
                                                         double* __restrict__ out) {
  __shared__ double s[W][256];
  double v[W];
#pragma unroll
  for (int q = 0; q < W; ++q) v[q] = threadIdx.x < blocks ? partial[size_t(threadIdx.x) * W + q] : 0.0;
  seg_block_tree<W>(s, v, out);
}

}  // namespace fdm
