// fdm_normals.hpp — surface normals and GICP covariances of a cloud by k-NN PCA, on the device.  gfx950 only.
//
// Reference being reproduced: nanoPCL geometry::estimateNormals / estimateCovariances / estimateNormalsCovariances in
// their k-NN form (geometry/normal_estimation.hpp:43-63, 107-124, 159-179; impl/normal_estimation_impl.hpp:33-68;
// impl/pca.hpp:34-107; impl/setters.hpp:20-105).  Per point: its k nearest points of the whole cloud, ITSELF INCLUDED,
// in ascending order; the first is the offset; sequential fp32 sums of d = p - offset and of d dT over them;
// cov = (sum_sq - (sum sumT) * inv_n) * inv_n; trace < FLT_EPSILON is degenerate; computeDirect (eig3_direct_all,
// fdm_post.hpp); normal = column 0, turned towards the viewpoint; covariance = V diag(1e-3, 1, 1) VT.
//
// The search is fdm_knn.hpp's: the same column grid (built by the same host routine), the same walk over rings of
// columns (knn_walk) with its stopping bound, the same queue for the lanes that are not settled after kKnnShells rings.
// What differs is the top-k, which keeps who as well as how far: one 64-bit key per slot, the squared distance's bits in
// the high word (it is >= +0, so its bits order it) and the point's INPUT index in the low word, compared as one
// integer — the (d2, index) order.  Where distances tie, that index order is this project's definition (nanoflann's
// follows its tree traversal); a tie can never straddle the stopping bound, which is strict.
//   k_nrm_search   one lane per query in sorted order; a settled lane gathers its neighbours' coordinates by input index,
//                  takes the sums, solves and writes at the query's input index (the PCA is fused: DESIGN.md §7)
//   k_nrm_brute    one block per queued query over the whole cloud: per-lane top-k of keys, merged through LDS in k
//                  rounds; every round's winner is the next neighbour, so the sums are taken as the merge goes
//   k_nrm_invalid  every point the invalid value (fewer than 3 neighbours)
// Invalid points are counted with one atomic per wavefront.  Every loop bound is known on the host before launch, as in
// fdm_knn.hpp.
#pragma once

#include "fdm_knn.hpp"
#include "fdm_post.hpp"

namespace fdm {

constexpr int kNrmBruteThreads = 128;
constexpr int kNrmMinNeighbors = 3;                 // MIN_NEIGHBORS (normal_estimation_impl.hpp:20)
constexpr unsigned long long kNrmEmpty = ~0ull;     // a slot that holds nobody: above every key (its high word is a NaN)
constexpr float kNrmGicpEpsilon = 1e-3f;            // GICP_EPSILON (setters.hpp:20)

struct NrmOut {
  float *nx, *ny, *nz;  // all three or none
  float* cov9;          // nullable; 9 floats per point, column-major
  float vx, vy, vz;     // the viewpoint
};

__device__ __forceinline__ unsigned long long nrm_key(float d2, float w) {
  return (static_cast<unsigned long long>(__float_as_uint(d2)) << 32) | __float_as_uint(w);
}

// The k smallest keys seen, ascending, in slots [KB - k, KB); the slots below hold 0, which no key is below (KnnTop's
// layout: every index a compile-time constant, the array stays in registers)
template <int KB>
struct NrmTop {
  unsigned long long v[KB];
  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int j = 0; j < KB; ++j) v[j] = j < KB - k ? 0ull : kNrmEmpty;
  }
  // the k-th squared distance; NaN (below no bound) while fewer than k are held
  __device__ __forceinline__ float kth() const { return __uint_as_float(uint32_t(v[KB - 1] >> 32)); }
  __device__ __forceinline__ void offer(float d2, float w) { push(nrm_key(d2, w)); }
  __device__ __forceinline__ void push(unsigned long long key) {
    if (key < v[KB - 1]) {
      v[KB - 1] = key;
#pragma unroll
      for (int j = KB - 1; j > 0; --j) {
        const unsigned long long a = v[j - 1], b = v[j];
        const bool sw = b < a;
        v[j - 1] = sw ? b : a;
        v[j] = sw ? a : b;
      }
    }
  }
};

// computeMeanAndCovariance's sums (pca.hpp:41-51): `first` sets the offset
struct NrmSums {
  float o[3], s[3], q[9];
  __device__ __forceinline__ void add(float px, float py, float pz, bool first) {
    if (first) {
      o[0] = px; o[1] = py; o[2] = pz;
#pragma unroll
      for (int a = 0; a < 3; ++a) s[a] = 0.0f;
#pragma unroll
      for (int a = 0; a < 9; ++a) q[a] = 0.0f;
    }
    const float d[3] = {px - o[0], py - o[1], pz - o[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] += d[a];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r) q[c * 3 + r] += d[r] * d[c];
  }
};

__device__ __forceinline__ void nrm_store_invalid(const NrmOut& O, size_t i) {  // setInvalid (setters.hpp:32, :59, :85)
  if (O.nx) { O.nx[i] = 0.0f; O.ny[i] = 0.0f; O.nz[i] = 0.0f; }
  if (O.cov9) {
#pragma unroll
    for (int a = 0; a < 9; ++a) O.cov9[i * 9 + size_t(a)] = (a % 4 == 0) ? 1.0f : 0.0f;
  }
}

// pca.hpp:53-55, computePCA (:67-88) and the setter (setters.hpp:37-48, :65-71) for the point (px, py, pz) at input index
// i with the sums of its m neighbours; false = the point got the invalid value.  Three-term dots are a0 b0 + (a1 b1 +
// a2 b2), the order the solver's own have (ASSUMED: DESIGN.md §6), as is the reading (sum sumT) * inv_n of pca.hpp:55.
__device__ __forceinline__ bool nrm_finish(const NrmSums& A, int m, float px, float py, float pz, const NrmOut& O,
                                           size_t i) {
  const float inv_n = 1.0f / float(m);
  float cov[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) cov[c * 3 + r] = (A.q[c * 3 + r] - (A.s[r] * A.s[c]) * inv_n) * inv_n;
  const float trace = cov[0] + cov[4] + cov[8];
  if (trace < 1.1920929e-07f) {
    nrm_store_invalid(O, i);
    return false;
  }
  float val[3], V[9];
  eig3_direct_all(cov, val, V);
  if (O.nx) {
    const float t[3] = {O.vx - px, O.vy - py, O.vz - pz};
    const float dot = V[0] * t[0] + (V[1] * t[1] + V[2] * t[2]);
    const bool flip = dot < 0.0f;
    O.nx[i] = flip ? -V[0] : V[0];
    O.ny[i] = flip ? -V[1] : V[1];
    O.nz[i] = flip ? -V[2] : V[2];
  }
  if (O.cov9) {
    float W[9];  // V * diag(1e-3, 1, 1), evaluated before the second product
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      W[r] = V[r] * kNrmGicpEpsilon;
      W[3 + r] = V[3 + r] * 1.0f;
      W[6 + r] = V[6 + r] * 1.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r)
        O.cov9[i * 9 + size_t(c * 3 + r)] = W[r] * V[c] + (W[3 + r] * V[3 + c] + W[6 + r] * V[6 + c]);
  }
  return true;
}

template <int KB>
__global__ __launch_bounds__(256) void k_nrm_search(unsigned n, int k, const float4* __restrict__ pts,
                                                    const uint32_t* __restrict__ start, const KnnGrid G,
                                                    const float* __restrict__ x, const float* __restrict__ y,
                                                    const float* __restrict__ z, const NrmOut O,
                                                    uint32_t* __restrict__ queue, KnnStat* __restrict__ st) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  bool invalid = false;  // (no early return: the count below is taken by whole wavefronts)
  if (p < n) {
    const float4 q = pts[p];
    NrmTop<KB> top;
    top.init(k);
    if (knn_walk<true>(p, q, pts, start, G, top)) {
      NrmSums A;
#pragma unroll
      for (int j = 0; j < KB; ++j)
        if (j >= KB - k) {
          // (a settled lane holds k points: k <= n and the whole cloud is the candidate set; the clamp keeps a slot that
          // held nobody from becoming an address all the same)
          const uint32_t t = min(uint32_t(top.v[j]), n - 1u);
          A.add(x[t], y[t], z[t], j == KB - k);
        }
      invalid = !nrm_finish(A, k, q.x, q.y, q.z, O, size_t(__float_as_uint(q.w)));
    } else {
      queue[atomicAdd(&st->n_queue, 1u)] = p;
    }
  }
  const unsigned long long mb = __ballot(invalid);
  if ((threadIdx.x & 63u) == 0u && mb) atomicAdd(&st->n_invalid, unsigned(__popcll(mb)));
}

// block b resolves the query at sorted position queue[b] against every point
template <int KB>
__global__ __launch_bounds__(kNrmBruteThreads) void k_nrm_brute(const uint32_t* __restrict__ queue, unsigned n, int k,
                                                                const float4* __restrict__ pts,
                                                                const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ z, const NrmOut O,
                                                                KnnStat* __restrict__ st) {
  __shared__ unsigned long long s_v[KB][kNrmBruteThreads];
  __shared__ unsigned long long s_best[kNrmBruteThreads / 64];
  const unsigned tid = threadIdx.x;
  const unsigned p = queue[blockIdx.x];
  const float4 q = pts[p];
  NrmTop<KB> top;
  top.init(k);
#pragma unroll 1
  for (unsigned t = tid; t < n; t += unsigned(kNrmBruteThreads)) {
    const float4 c = pts[t];
    top.offer(knn_dist2(q, c), c.w);
  }
#pragma unroll
  for (int j = 0; j < KB; ++j) s_v[j][tid] = top.v[j];
  // k rounds: the smallest head among the lanes' ascending lists is the next neighbour (keys are distinct: the index is
  // part of them), its lane moves on.  Every lane takes the same sums.
  int head = KB - k;
  NrmSums A{};
#pragma unroll 1
  for (int r = 0; r < k; ++r) {
    const unsigned long long mine = head < KB ? s_v[head][tid] : kNrmEmpty;
    unsigned long long key = mine;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const unsigned long long o = __shfl_xor(key, s);
      key = o < key ? o : key;
    }
    if ((tid & 63u) == 0u) s_best[tid >> 6] = key;
    __syncthreads();
    unsigned long long best = s_best[0];
#pragma unroll
    for (int w = 1; w < kNrmBruteThreads / 64; ++w) best = s_best[w] < best ? s_best[w] : best;
    __syncthreads();
    if (best == kNrmEmpty) break;  // (fewer than k points: the host never asks for that)
    if (mine == best) ++head;
    const uint32_t t = min(uint32_t(best), n - 1u);
    A.add(x[t], y[t], z[t], r == 0);
  }
  if (tid == 0u && !nrm_finish(A, k, q.x, q.y, q.z, O, size_t(__float_as_uint(q.w)))) atomicAdd(&st->n_invalid, 1u);
}

inline __global__ __launch_bounds__(256) void k_nrm_invalid(unsigned n, const NrmOut O) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) nrm_store_invalid(O, size_t(i));
}

}  // namespace fdm
