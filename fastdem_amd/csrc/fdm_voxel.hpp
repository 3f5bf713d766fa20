// fdm_voxel.hpp — the cloud downsampling filters nanopcl::filters::voxelGrid (all four modes) and gridMaxZ on the device:
// the kernels behind fdm_cloud_voxel_grid / fdm_cloud_grid_max_z (host side: fdm_engine_voxel.inl).  gfx950 only.
//
// Reference being served:
//   lib/nanoPCL/include/nanopcl/filters/impl/voxel_grid_impl.hpp:30-236   voxelGrid: keys, std::sort, one output per run
//   lib/nanoPCL/include/nanopcl/filters/impl/grid_max_z_impl.hpp:31-75    gridMaxZ: the key of (x, y, 0), first largest z
//   lib/nanoPCL/include/nanopcl/core/voxel.hpp:28-102                     pack, toCenter
//
// The keys (k_voxel_keys) and both sorts (fdm_rsort.hpp, fdm_introsort.hpp) are the raycasting stage's; what is here turns
// the sorted (key, index) pairs into a cloud:
//   k_vx_count   run heads (key differs from its predecessor, not the invalid key) per block of 256 sorted positions
//   k_pack_scan  (fdm_egress.hpp) exclusive scan of the block counts; its total is n_out
//   k_vx_heads   pos[slot] = sorted position of the slot's run head (slot = block offset + rank in the block), pos[n_out] =
//                number of valid entries, so run r is [pos[r], pos[r + 1]); and the channels a mode walks, gathered ONCE
//                into sorted order by one lane per sorted position (coalesced idx, gathered value, coalesced store)
//   k_vx_reduce  one lane per RUN (slots are dense: no idle lanes between heads): the fp32 sums of a run are a contract —
//                from 0, in the run's order, no reassociation — so they are one dependency chain per channel; the loads
//                are consecutive addresses of the staged arrays, issued kVxBatch entries ahead of the chains
//   k_vx_reduce_long   runs of more than kVxLong entries, one WAVEFRONT each: 64 entries per coalesced load, the chains
//                fed by readlane; NEAREST / gridMaxZ, whose result does not depend on the order of evaluation, as a
//                wavefront reduction
// The sums of a cloud that falls into ONE voxel stay a serial walk (as in the reference).
#pragma once

#include "fdm_raycast.hpp"

namespace fdm {

// VoxelMode's enum order (filters/downsample.hpp), then gridMaxZ
constexpr int kVxCentroid = 0, kVxNearest = 1, kVxAny = 2, kVxCenter = 3, kVxMaxZ = 4;

struct VxCloud {  // SoA input; x, y, z always, the rest nullable
  const float *x, *y, *z, *intensity;
  const uint32_t* rgb;  // 0x00RRGGBB
  const float *nx, *ny, *nz;
  const float* cov9;    // 9 floats per point
};
struct VxOut {  // any may be null
  float *x, *y, *z, *intensity;
  uint32_t* rgb;
  float *nx, *ny, *nz;
  float* cov9;
  uint32_t* idx;
};
struct VxStage {  // the channels a mode walks, in sorted order (null: not walked)
  float *x, *y, *z, *intensity;
  uint32_t* rgb;
  float *nx, *ny, *nz;
};

__device__ __forceinline__ bool vx_head(const unsigned long long* __restrict__ keys, unsigned i, unsigned n) {
  if (i >= n) return false;
  const unsigned long long k = keys[i];
  return k != kInvalidVoxel && (i == 0u || keys[i - 1u] != k);
}

inline __global__ __launch_bounds__(256) void k_vx_count(unsigned n, const unsigned long long* __restrict__ keys,
                                                         uint32_t* __restrict__ counts) {
  __shared__ unsigned s_w[4];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned long long m = __ballot(vx_head(keys, i, n));
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = unsigned(__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0u) counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// offsets: k_vx_count's counts after k_pack_scan (offsets[gridDim.x] = n_out); pos has n + 1 entries
inline __global__ __launch_bounds__(256) void k_vx_heads(unsigned n, const unsigned long long* __restrict__ keys,
                                                         const uint32_t* __restrict__ idx,
                                                         const uint32_t* __restrict__ offsets, const VxCloud C,
                                                         const VxStage S, uint32_t* __restrict__ pos) {
  __shared__ unsigned s_w[4];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const bool in = i < n;
  const unsigned long long k = in ? keys[i] : kInvalidVoxel;
  const unsigned long long p = (in && i > 0u) ? keys[i - 1u] : kInvalidVoxel;
  const bool valid = k != kInvalidVoxel;
  const bool head = valid && (i == 0u || p != k);
  const unsigned long long m = __ballot(head);
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0u) s_w[w] = unsigned(__popcll(m));
  __syncthreads();
  if (head) {
    unsigned rank = unsigned(__popcll(m & ((1ull << lane) - 1ull)));
    for (unsigned q = 0; q < w; ++q) rank += s_w[q];
    pos[offsets[blockIdx.x] + rank] = i;
  }
  // the end of the last run: the first invalid entry behind a valid one, or n
  if (in && !valid && i > 0u && p != kInvalidVoxel) pos[offsets[gridDim.x]] = i;
  if (in && valid && i == n - 1u) pos[offsets[gridDim.x]] = n;
  if (!valid) return;
  const uint32_t o = idx[i];
  if (S.x) S.x[i] = C.x[o];
  if (S.y) S.y[i] = C.y[o];
  if (S.z) S.z[i] = C.z[o];
  if (S.intensity) S.intensity[i] = C.intensity[o];
  if (S.rgb) S.rgb[i] = C.rgb[o];
  if (S.nx) { S.nx[i] = C.nx[o]; S.ny[i] = C.ny[o]; S.nz[i] = C.nz[o]; }
}

// every channel of input point `from` into output slot r
__device__ __forceinline__ void vx_copy_point(const VxCloud& C, const VxOut& O, unsigned r, uint32_t from) {
  if (O.x) O.x[r] = C.x[from];
  if (O.y) O.y[r] = C.y[from];
  if (O.z) O.z[r] = C.z[from];
  if (O.intensity && C.intensity) O.intensity[r] = C.intensity[from];
  if (O.rgb && C.rgb) O.rgb[r] = C.rgb[from];
  if (C.nx) {  // (the input's three arrays come together; every output array is optional on its own)
    if (O.nx) O.nx[r] = C.nx[from];
    if (O.ny) O.ny[r] = C.ny[from];
    if (O.nz) O.nz[r] = C.nz[from];
  }
  if (O.cov9 && C.cov9)
    for (int q = 0; q < 9; ++q) O.cov9[size_t(r) * 9u + q] = C.cov9[size_t(from) * 9u + q];
  if (O.idx) O.idx[r] = from;
}

// voxel::toCenter of one axis field of the key (voxel.hpp:65-91)
__device__ __forceinline__ float vx_center(unsigned long long key, int shift, float size) {
  const int32_t i = int32_t((key >> shift) & 0x1FFFFFull) - (1 << 20);
  return (float(i) + 0.5f) * size;
}

// ---- the walks.  NEAREST and gridMaxZ keep the FIRST best entry of a run, i.e. the smallest (score, position) pair: an
// order-free reduction.  The sums of CENTROID and CENTER are not: one chain per channel, in the run's order. ----
constexpr unsigned kVxLong = 128u;   // runs longer than this leave k_vx_reduce for k_vx_reduce_long: a wavefront each
constexpr unsigned kVxBatch = 4u;    // entries a lane loads ahead of its chains (the loads are what a short walk waits for)

struct VxSums {  // a run's channel sums (the colour's as r, g, b)
  float x = 0.0f, y = 0.0f, z = 0.0f, i = 0.0f, r = 0.0f, g = 0.0f, b = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
};
struct VxVals {  // one sorted entry's summands; absent channels 0
  float x, y, z, i, r, g, b, nx, ny, nz;
};
template <int MODE>
__device__ __forceinline__ VxVals vx_load(const VxStage& S, unsigned j) {
  VxVals v{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (MODE == kVxCentroid) { v.x = S.x[j]; v.y = S.y[j]; v.z = S.z[j]; }
  if (S.intensity) v.i = S.intensity[j];
  if (S.rgb) {
    const uint32_t c = S.rgb[j];
    v.r = float((c >> 16) & 255u); v.g = float((c >> 8) & 255u); v.b = float(c & 255u);
  }
  if (S.nx) { v.nx = S.nx[j]; v.ny = S.ny[j]; v.nz = S.nz[j]; }
  return v;
}
template <int MODE>
__device__ __forceinline__ void vx_add(VxSums& a, const VxVals& v, const VxStage& S) {
  if (MODE == kVxCentroid) { a.x += v.x; a.y += v.y; a.z += v.z; }
  if (S.intensity) a.i += v.i;
  if (S.rgb) { a.r += v.r; a.g += v.g; a.b += v.b; }
  if (S.nx) { a.nx += v.nx; a.ny += v.ny; a.nz += v.nz; }
}
__device__ __forceinline__ float vx_lane(float v, unsigned k) {  // lane k's v, k uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), int(k)));
}

// CENTROID (:98-140) and CENTER (:191-229) of run [i0, end) into slot r: every sum divided by float(count)
template <int MODE>
__device__ __forceinline__ void vx_emit_mean(const VxSums& a, unsigned i0, unsigned end, unsigned r,
                                             const unsigned long long* __restrict__ keys,
                                             const uint32_t* __restrict__ idx, const VxCloud& C, const VxStage& S,
                                             float size, const VxOut& O) {
  const float cnt = float(end - i0);
  if (MODE == kVxCentroid) {
    if (O.x) O.x[r] = a.x / cnt;
    if (O.y) O.y[r] = a.y / cnt;
    if (O.z) O.z[r] = a.z / cnt;
  } else {
    const unsigned long long key = keys[i0];
    if (O.x) O.x[r] = vx_center(key, 0, size);
    if (O.y) O.y[r] = vx_center(key, 21, size);
    if (O.z) O.z[r] = vx_center(key, 42, size);
  }
  if (O.intensity && S.intensity) O.intensity[r] = a.i / cnt;
  if (O.rgb && S.rgb) {  // static_cast<uint8_t>(float): truncated, low eight bits
    const uint32_t cr = uint32_t(int(a.r / cnt)) & 255u, cg = uint32_t(int(a.g / cnt)) & 255u, cb = uint32_t(int(a.b / cnt)) & 255u;
    O.rgb[r] = (cr << 16) | (cg << 8) | cb;
  }
  if (S.nx) {
    const float norm = sqrtf((a.nx * a.nx + a.ny * a.ny) + a.nz * a.nz);
    const bool ok = norm > 1e-6f;
    if (O.nx) O.nx[r] = ok ? a.nx / norm : 0.0f;
    if (O.ny) O.ny[r] = ok ? a.ny / norm : 0.0f;
    if (O.nz) O.nz[r] = ok ? a.nz / norm : 1.0f;
  }
  const uint32_t rep = idx[i0];
  if (O.cov9 && C.cov9)
    for (int q = 0; q < 9; ++q) O.cov9[size_t(r) * 9u + q] = C.cov9[size_t(rep) * 9u + q];
  if (O.idx) O.idx[r] = rep;
}

// what NEAREST (d2 to the voxel's centre, smaller is better) and gridMaxZ (-z) minimise, at sorted position j
template <int MODE>
__device__ __forceinline__ float vx_score(const VxStage& S, unsigned j, float cx, float cy, float cz) {
  if (MODE == kVxMaxZ) return -S.z[j];
  // :147, squaredNorm of the 4-vector (w: 1 - 1) as Eigen's packet reduction sums it
  const float dx = S.x[j] - cx, dy = S.y[j] - cy, dz = S.z[j] - cz;
  return (dx * dx + dz * dz) + (dy * dy + 0.0f);
}

// One lane per run.  long_count / long_list (null: walk every run here): the slots of the runs left to k_vx_reduce_long.
template <int MODE>
__global__ __launch_bounds__(256) void k_vx_reduce(unsigned n_out, const uint32_t* __restrict__ pos,
                                                   const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ idx, const VxCloud C, const VxStage S,
                                                   float size, const VxOut O, uint32_t* __restrict__ long_count,
                                                   uint32_t* __restrict__ long_list) {
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_out) return;
  const unsigned i0 = pos[r], end = pos[r + 1u];
  if (MODE == kVxAny) {  // voxel_grid_impl.hpp:171-173, size_t arithmetic
    const unsigned long long c = end - i0, s0 = i0;
    vx_copy_point(C, O, r, idx[i0 + unsigned((c * 7ull + s0 * 13ull) % c)]);
    return;
  }
  if (long_list && end - i0 > kVxLong) {
    long_list[atomicAdd(long_count, 1u)] = r;
    return;
  }
  if (MODE == kVxMaxZ || MODE == kVxNearest) {
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (MODE == kVxNearest) {
      const unsigned long long key = keys[i0];
      cx = vx_center(key, 0, size); cy = vx_center(key, 21, size); cz = vx_center(key, 42, size);
    }
    // grid_max_z_impl.hpp:58-67: the first strictly greater z, from the run's first; voxel_grid_impl.hpp:144-152: the
    // first strictly smaller d2, from FLT_MAX with the rep
    float best = MODE == kVxMaxZ ? vx_score<MODE>(S, i0, cx, cy, cz) : 3.402823466e+38f;
    unsigned at = i0;
    for (unsigned j = i0; j < end; j += kVxBatch) {
      float sc[kVxBatch];
#pragma unroll
      for (unsigned u = 0; u < kVxBatch; ++u) sc[u] = vx_score<MODE>(S, min(j + u, end - 1u), cx, cy, cz);
#pragma unroll
      for (unsigned u = 0; u < kVxBatch; ++u)
        if (j + u < end && sc[u] < best) { best = sc[u]; at = j + u; }
    }
    vx_copy_point(C, O, r, idx[at]);
    return;
  }
  VxSums a;
  for (unsigned j = i0; j < end; j += kVxBatch) {
    VxVals v[kVxBatch];
#pragma unroll
    for (unsigned u = 0; u < kVxBatch; ++u) v[u] = vx_load<MODE>(S, min(j + u, end - 1u));
#pragma unroll
    for (unsigned u = 0; u < kVxBatch; ++u)
      if (j + u < end) vx_add<MODE>(a, v[u], S);
  }
  vx_emit_mean<MODE>(a, i0, end, r, keys, idx, C, S, size, O);
}

// One wavefront per long run (grid-stride over the list).  Sums: the wavefront loads 64 consecutive entries at once, one
// per lane, and every lane adds them up in order (lane k's value by readlane: the same chain in every lane), the next 64
// already on their way.  NEAREST / gridMaxZ: every lane keeps the first best of its stride, the wavefront the smallest
// (score, position) of them.
template <int MODE>
__global__ __launch_bounds__(64) void k_vx_reduce_long(const uint32_t* __restrict__ long_count,
                                                       const uint32_t* __restrict__ long_list,
                                                       const uint32_t* __restrict__ pos,
                                                       const unsigned long long* __restrict__ keys,
                                                       const uint32_t* __restrict__ idx, const VxCloud C, const VxStage S,
                                                       float size, const VxOut O) {
  const unsigned lane = threadIdx.x;
  const unsigned n_long = *long_count;
  for (unsigned q = blockIdx.x; q < n_long; q += gridDim.x) {
    const unsigned r = long_list[q];
    const unsigned i0 = pos[r], end = pos[r + 1u];
    if (MODE == kVxMaxZ || MODE == kVxNearest) {
      float cx = 0.0f, cy = 0.0f, cz = 0.0f;
      if (MODE == kVxNearest) {
        const unsigned long long key = keys[i0];
        cx = vx_center(key, 0, size); cy = vx_center(key, 21, size); cz = vx_center(key, 42, size);
      }
      // (a lane without a candidate holds (FLT_MAX, rep): NEAREST's start.  gridMaxZ's scores are finite: below it)
      float best = 3.402823466e+38f;
      unsigned at = i0;
      for (unsigned j = i0 + lane; j < end; j += 64u) {
        const float sc = vx_score<MODE>(S, j, cx, cy, cz);
        if (sc < best) { best = sc; at = j; }
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float ob = __shfl_xor(best, d);
        const unsigned oa = __shfl_xor(at, d);
        if (ob < best || (ob == best && oa < at)) { best = ob; at = oa; }
      }
      if (lane == 0u) vx_copy_point(C, O, r, idx[at]);
      continue;
    }
    if (MODE == kVxCentroid || MODE == kVxCenter) {
      const VxVals zero{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      VxSums a;
      VxVals cur = i0 + lane < end ? vx_load<MODE>(S, i0 + lane) : zero;
      for (unsigned base = i0; base < end; base += 64u) {
        const unsigned nj = base + 64u + lane;
        const VxVals nxt = nj < end ? vx_load<MODE>(S, nj) : zero;
        const unsigned m = min(64u, end - base);
        for (unsigned k = 0; k < m; ++k) {
          if (MODE == kVxCentroid) { a.x += vx_lane(cur.x, k); a.y += vx_lane(cur.y, k); a.z += vx_lane(cur.z, k); }
          if (S.intensity) a.i += vx_lane(cur.i, k);
          if (S.rgb) { a.r += vx_lane(cur.r, k); a.g += vx_lane(cur.g, k); a.b += vx_lane(cur.b, k); }
          if (S.nx) { a.nx += vx_lane(cur.nx, k); a.ny += vx_lane(cur.ny, k); a.nz += vx_lane(cur.nz, k); }
        }
        cur = nxt;
      }
      if (lane == 0u) vx_emit_mean<MODE>(a, i0, end, r, keys, idx, C, S, size, O);
    }
  }
}

}  // namespace fdm
