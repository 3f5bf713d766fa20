// fdm_knn.hpp — exact k-nearest-neighbour mean distances for statistical outlier removal, on the device.  gfx950 only.
//
// Reference being reproduced: lib/nanoPCL/include/nanopcl/filters/impl/outlier_removal_impl.hpp:83-142.  Per point the
// mean of the sqrt of the k smallest squared distances to the OTHER points (duplicates count, at distance 0), summed in
// ascending order in fp32.  The global mean / deviation of those means are two fp64 sums in input order and are taken
// on the host (fdm_engine_dem.inl) — a tree reduction rounds differently.
//
// The search is exact.  Points are grouped into square COLUMNS of the x / y plane (a DEM cloud is a surface: its points
// per column do not grow with the height range, and the table of column starts is bounded by the footprint, which a
// table of 3-D voxels is not):
//   k_knn_bounds  x / y bounding box (ordered-key atomics) and the flag word: some coordinate is not finite
//   k_knn_keys    key = cy * gx + cx, cx = min(int((x - min_x) * inv_h), gx - 1): monotone in x whatever the rounding
//   fdm_rsort     stable sort of (key, point index)
//   k_knn_gather  the points in sorted order, one float4 each (w = the point's index)
//   k_knn_starts  start[c] = lower bound of c in the sorted keys, c = 0 .. gx * gy: a row of columns is ONE range
//   k_knn_search  one lane per query, in sorted order (neighbouring lanes read the same columns): a sorted top-k in
//                 registers, rings of columns outward.  After ring s every unvisited point is at least
//                 (s + margin) * h away in x or in y, margin = the query's distance to the nearest face of its own
//                 column; the search stops when k candidates are held and the k-th squared distance is below the
//                 square of that bound, which is first made smaller by 2^-8 columns (the two roundings of `u` are
//                 below 2^-10 columns at 2 048 columns per axis) and by two factors of 0.9999 (the roundings of the
//                 squared distance are below 2^-22 relative).  A lane that is not done after kKnnShells rings — an
//                 isolated outlier, the very thing SOR looks for — appends itself to a queue.
//   k_knn_brute   one block per queued query over the whole cloud: per-lane top-k, merged in LDS
// fdm_normals.hpp searches the same grid with the same walk (knn_walk) and keeps who the neighbours are as well.
// Every loop bound is known on the host before launch: kKnnShells rings, runs of at most n points, at most n queue
// entries, k rounds of the merge.
#pragma once

#include "fdm_device.hpp"

namespace fdm {

constexpr int kKnnMaxK = 64;             // effective_k above this is refused (fdm_statistical_outlier_removal)
constexpr int kKnnShells = 4;            // rings a query lane visits (a 9 x 9 block of columns) before it queues itself
constexpr unsigned kKnnGridMax = 2048u;  // columns per axis: 22-bit keys, a table of at most 4 M + 1 starts
constexpr int kKnnBruteThreads = 128;

struct KnnStat {
  uint32_t min_x, min_y, max_x, max_y;  // ord() of the bounding box
  uint32_t nonfinite;                   // some x, y or z is NaN or infinite
  uint32_t n_queue;                     // queries left to k_knn_brute
  uint32_t n_kept;                      // k_sor_keep
  uint32_t n_invalid;                   // points that got the invalid value (fdm_normals.hpp)
};
struct KnnGrid {
  float min_x, min_y, inv_h, h;
  int gx, gy;
};

inline __global__ void k_knn_init(KnnStat* __restrict__ st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->min_x = st->min_y = 0xFFFFFFFFu;
    st->max_x = st->max_y = 0u;
    st->nonfinite = st->n_queue = st->n_kept = st->n_invalid = 0u;
  }
}

inline __global__ __launch_bounds__(256) void k_knn_bounds(unsigned n, const float* __restrict__ x,
                                                           const float* __restrict__ y, const float* __restrict__ z,
                                                           KnnStat* __restrict__ st) {
  uint32_t a = 0xFFFFFFFFu, b = 0xFFFFFFFFu, c = 0u, d = 0u;
  bool bad = false;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const float px = x[i], py = y[i], pz = z[i];
    if (!(fabsf(px) <= kFltMax) || !(fabsf(py) <= kFltMax) || !(fabsf(pz) <= kFltMax)) { bad = true; continue; }
    const uint32_t ox = ord(px), oy = ord(py);
    a = min(a, ox); b = min(b, oy);
    c = max(c, ox); d = max(d, oy);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    a = min(a, uint32_t(__shfl_xor(int(a), s)));
    b = min(b, uint32_t(__shfl_xor(int(b), s)));
    c = max(c, uint32_t(__shfl_xor(int(c), s)));
    d = max(d, uint32_t(__shfl_xor(int(d), s)));
  }
  const unsigned long long mb = __ballot(bad);
  if ((threadIdx.x & 63u) == 0u) {
    atomicMin(&st->min_x, a); atomicMin(&st->min_y, b);
    atomicMax(&st->max_x, c); atomicMax(&st->max_y, d);
    if (mb) atomicOr(&st->nonfinite, 1u);
  }
}

// column coordinate of a point (p >= mn): the same two roundings wherever a column is computed
__device__ __forceinline__ float knn_u(float p, float mn, float inv_h) { return __fmul_rn(__fsub_rn(p, mn), inv_h); }
__device__ __forceinline__ int knn_col(float u, int g) {
  const int c = int(u);
  return c > g - 1 ? g - 1 : (c < 0 ? 0 : c);
}

inline __global__ __launch_bounds__(256) void k_knn_keys(unsigned n, const float* __restrict__ x,
                                                         const float* __restrict__ y, const KnnGrid G,
                                                         uint32_t* __restrict__ keys) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int cx = knn_col(knn_u(x[i], G.min_x, G.inv_h), G.gx);
  const int cy = knn_col(knn_u(y[i], G.min_y, G.inv_h), G.gy);
  keys[i] = uint32_t(cy) * uint32_t(G.gx) + uint32_t(cx);
}

inline __global__ __launch_bounds__(256) void k_knn_gather(unsigned n, const uint32_t* __restrict__ idx,
                                                           const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ z, float4* __restrict__ pts) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n) return;
  const uint32_t i = idx[p];
  pts[p] = make_float4(x[i], y[i], z[i], __uint_as_float(i));
}

// start[c] = number of sorted keys below c, c = 0 .. ncol (start[ncol] = n): 32 halving steps at the most
inline __global__ __launch_bounds__(256) void k_knn_starts(unsigned n, const uint32_t* __restrict__ skeys,
                                                           unsigned ncol, uint32_t* __restrict__ start) {
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  if (c > ncol) return;
  unsigned lo = 0u, hi = n;
#pragma unroll 1
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] < c) lo = mid + 1u; else hi = mid;
  }
  start[c] = lo;
}

// ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded on its own (the reference builds without FMA)
__device__ __forceinline__ float knn_dist2(const float4& a, const float4& b) {
  const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y), dz = __fsub_rn(a.z, b.z);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// The k smallest values seen, ascending, in slots [KB - k, KB); the slots below hold -1 (smaller than any squared
// distance) so that the k-th best is always slot KB - 1 and every index is a compile-time constant: the array stays in
// registers.
template <int KB>
struct KnnTop {
  float v[KB];
  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int j = 0; j < KB; ++j) v[j] = j < KB - k ? -1.0f : __builtin_inff();
  }
  __device__ __forceinline__ float kth() const { return v[KB - 1]; }
  __device__ __forceinline__ void offer(float d, float /*w*/) { push(d); }  // what knn_walk calls: who is not kept
  __device__ __forceinline__ void push(float d) {
    if (d < v[KB - 1]) {
      v[KB - 1] = d;
#pragma unroll
      for (int j = KB - 1; j > 0; --j) {
        const float a = v[j - 1], b = v[j];
        const bool sw = b < a;
        v[j - 1] = sw ? b : a;
        v[j] = sw ? a : b;
      }
    }
  }
  // (sum of sqrt in ascending order) / k: outlier_removal_impl.hpp:106-115.  sqrtf, not __fsqrt_rn: the library is
  // built with -fhip-fp32-correctly-rounded-divide-sqrt, which makes sqrtf the correctly rounded one, while the
  // intrinsic is the hardware's approximate square root
  __device__ __forceinline__ float mean(int k) const {
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < KB; ++j)
      if (j >= KB - k) sum = __fadd_rn(sum, sqrtf(v[j]));
    return __fdiv_rn(sum, float(k));
  }
};

// The query at sorted position p walks rings of columns outward and offers every point it meets — itself too when SELF —
// to `top` (offer(d2, w), kth()).  True once `top` holds the k nearest of the whole cloud: the whole grid was seen, or the
// k-th squared distance is below the square of the ring's bound (the file comment); false after `rings` rings.
// RADIUS (fdm_register.hpp: the query is no member of the grid and may lie outside its box — knn_col clamps and the margin
// falls to 0, which only makes the bound more conservative): the walk also ends, true, once that bound's square exceeds
// max_d2 — no unvisited point can then be within the radius — and the host picks `rings` so that one of the exits is
// always taken.  The defaults are the walk of the k-NN kernels, unchanged.
template <bool SELF, class Top, bool RADIUS = false>
__device__ __forceinline__ bool knn_walk(unsigned p, const float4& q, const float4* __restrict__ pts,
                                         const uint32_t* __restrict__ start, const KnnGrid& G, Top& top,
                                         int rings = kKnnShells, float max_d2 = 0.0f) {
  const float ux = knn_u(q.x, G.min_x, G.inv_h), uy = knn_u(q.y, G.min_y, G.inv_h);
  const int cx = knn_col(ux, G.gx), cy = knn_col(uy, G.gy);
  float margin;
  {
    const float fx = ux - float(cx), fy = uy - float(cy);
    margin = fminf(fminf(fx, 1.0f - fx), fminf(fy, 1.0f - fy));
    margin = margin > 0.0f ? margin : 0.0f;
  }
  bool done = false;
#pragma unroll 1
  for (int s = 0; s <= rings && !done; ++s) {
    const int y0 = cy - s < 0 ? 0 : cy - s, y1 = cy + s > G.gy - 1 ? G.gy - 1 : cy + s;
    const int x0 = cx - s < 0 ? 0 : cx - s, x1 = cx + s > G.gx - 1 ? G.gx - 1 : cx + s;
#pragma unroll 1
    for (int yy = y0; yy <= y1; ++yy) {
      const unsigned row = unsigned(yy) * unsigned(G.gx);
      const bool full = yy == cy - s || yy == cy + s;  // a row of the ring's top or bottom edge: every column of it
#pragma unroll 1
      for (int part = 0; part < (full ? 1 : 2); ++part) {
        int xa, xb;
        if (full) { xa = x0; xb = x1; }
        else {  // the two end columns (s >= 1 here)
          xa = xb = part == 0 ? cx - s : cx + s;
          if (xa < 0 || xa > G.gx - 1) continue;
        }
        const unsigned t0 = start[row + unsigned(xa)], t1 = start[row + unsigned(xb) + 1u];
#pragma unroll 1
        for (unsigned t = t0; t < t1; ++t)
          if (SELF || t != p) {
            const float4 c = pts[t];
            top.offer(knn_dist2(q, c), c.w);
          }
      }
    }
    if (x0 == 0 && y0 == 0 && x1 == G.gx - 1 && y1 == G.gy - 1) { done = true; break; }  // the whole cloud was seen
    const float lb = __fmul_rn(__fmul_rn(float(s) + margin - 0.00390625f, G.h), 0.9999f);
    if (lb > 0.0f) {
      const float lb2 = __fmul_rn(__fmul_rn(lb, lb), 0.9999f);
      done = top.kth() < lb2 || (RADIUS && max_d2 < lb2);
    }
  }
  return done;
}

template <int KB>
__global__ __launch_bounds__(256) void k_knn_search(unsigned n, int k, const float4* __restrict__ pts,
                                                    const uint32_t* __restrict__ start, const KnnGrid G,
                                                    float* __restrict__ mean, uint32_t* __restrict__ queue,
                                                    KnnStat* __restrict__ st) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n) return;
  const float4 q = pts[p];
  KnnTop<KB> top;
  top.init(k);
  if (knn_walk<false>(p, q, pts, start, G, top)) mean[__float_as_uint(q.w)] = top.mean(k);
  else queue[atomicAdd(&st->n_queue, 1u)] = p;
}

// block b resolves the query at sorted position queue[b] against every other point
template <int KB>
__global__ __launch_bounds__(kKnnBruteThreads) void k_knn_brute(const uint32_t* __restrict__ queue, unsigned n, int k,
                                                                const float4* __restrict__ pts,
                                                                float* __restrict__ mean) {
  __shared__ float s_v[KB][kKnnBruteThreads];
  __shared__ unsigned long long s_best[kKnnBruteThreads / 64];
  const unsigned tid = threadIdx.x;
  const unsigned p = queue[blockIdx.x];
  const float4 q = pts[p];
  KnnTop<KB> top;
  top.init(k);
#pragma unroll 1
  for (unsigned t = tid; t < n; t += unsigned(kKnnBruteThreads))
    if (t != p) top.push(knn_dist2(q, pts[t]));
#pragma unroll
  for (int j = 0; j < KB; ++j) s_v[j][tid] = top.v[j];
  // k rounds: the smallest head among the lanes' ascending lists leaves, its lane moves on
  int head = KB - k;
  float sum = 0.0f;
#pragma unroll 1
  for (int r = 0; r < k; ++r) {
    const float mine = head < KB ? s_v[head][tid] : __builtin_inff();
    unsigned long long key = ((unsigned long long)__float_as_uint(mine) << 32) | tid;  // mine >= 0: its bits order it
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const unsigned long long o = __shfl_xor(key, s);
      key = o < key ? o : key;
    }
    if ((tid & 63u) == 0u) s_best[tid >> 6] = key;
    __syncthreads();
    unsigned long long best = s_best[0];
#pragma unroll
    for (int w = 1; w < kKnnBruteThreads / 64; ++w) best = s_best[w] < best ? s_best[w] : best;
    __syncthreads();
    if (unsigned(best & 0xFFFFFFFFull) == tid) ++head;
    sum = __fadd_rn(sum, sqrtf(__uint_as_float(uint32_t(best >> 32))));
  }
  if (tid == 0u) mean[__float_as_uint(q.w)] = __fdiv_rn(sum, float(k));
}

// keep[i] = mean[i] <= threshold (outlier_removal_impl.hpp:133-136)
inline __global__ __launch_bounds__(256) void k_sor_keep(unsigned n, const float* __restrict__ mean, float threshold,
                                                         uint8_t* __restrict__ keep, KnnStat* __restrict__ st) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const bool in = i < n && mean[i] <= threshold;
  if (i < n) keep[i] = in ? 1 : 0;
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&st->n_kept, unsigned(__popcll(m)));
}

}  // namespace fdm
