// fdm_vgicp.hpp — the voxel distribution map of voxelized GICP and the lookup-based linearization, on the device: the
// kernels behind fdm_voxel_map_create and fdm_cloud_register_vgicp (host side: fdm_engine_vgicp.inl).  gfx950 only, wave64.
//
// Reference being reproduced: nanoPCL registration::VoxelDistributionMap::build / lookupRegularized
// (registration/voxel_distribution_map.hpp:143-323), VoxelCorrespondence::find (correspondence/voxel_correspondence.hpp:
// 55-75), VGICPFactor = GICPFactor (factors/vgicp_factor.hpp) and alignVGICP (align.hpp:276-353); the key is voxel::pack
// (core/voxel.hpp:28-42).
//
// The map is built from the sorted (key, index) pairs fdm_voxel.hpp already knows how to make — k_voxel_keys, the STABLE
// radix sort, k_vx_count / k_pack_scan / k_vx_heads with x, y, z staged in sorted order — so a run is one voxel and its
// entries are in input order:
//   k_vg_reduce        one lane per run: nine double chains (the sums of p and of the six products p_a p_b, a float
//                      product held exactly by a double), the first entry ASSIGNED and the others added in the run's
//                      order — a contract: no reassociation, no floating-point atomics; the loads are issued kVgBatch
//                      entries ahead of the chains (as k_vx_reduce); then the record
//   k_vg_reduce_long   runs of more than kVxLong entries, one wavefront each: 64 entries per coalesced load, the chains
//                      fed by readlane, the same chain in every lane (as k_vx_reduce_long)
//   k_vg_insert        one lane per voxel: its key into an open-addressing table (linear probing from a mix of all 63
//                      key bits; the reference's `key & mask` leaves z out of any table under 2^42 slots) by a 64-bit
//                      atomicCAS — the keys are distinct, nothing is ever updated — and its rank beside it; the longest
//                      probe sequence by atomicMax
//   k_vg_linearize     k_reg_linearize's sibling: the same transform, then key, probe, record fetch, the GICP factor
//                      with q = double(mean) and C_tgt = the voxel's regularised covariance, the same block sum; the
//                      partials go through k_reg_reduce unchanged
// A record: key, count, mean (3 floats), cov (9 floats, column-major), C_reg (six doubles: xx, xy, xz, yy, yz, zz), in
// ascending key order; a voxel's rank in that order is what a correspondence names.  C_reg of a voxel of three or more
// points is reg_regularize_one's (fdm_register.hpp) of the stored float covariance; of a sparser one the identity.
//
// Every loop bound is known on the host before launch, the rule fdm_register.hpp states for its walk: an insertion
// probes at most `slots` times (the table is at most half full), a lookup at most max_probe times — the longest
// sequence any insertion took, read back by the host when the table is built and handed to every later launch.
#pragma once

#include "fdm_register.hpp"
#include "fdm_voxel.hpp"

namespace fdm {

constexpr unsigned long long kVgEmpty = ~0ull;  // no valid key has bit 63 set
constexpr unsigned kVgBatch = 4u;               // entries a lane loads ahead of its chains

struct VgRecords {  // num_voxels entries each, ascending key
  unsigned long long* key;
  uint32_t* count;
  float* mean3;
  float* cov9;
  double* creg6;
};
struct VgStat {  // zeroed before the build
  uint32_t n_sparse;    // voxels of fewer than three points
  uint32_t max_count;   // the fullest voxel's points
  uint32_t max_probe;   // slots the longest insertion looked at
  uint32_t long_count;  // runs left to k_vg_reduce_long
};
struct VgTable {  // what a lookup reads
  const unsigned long long* slot_key;  // slots entries, kVgEmpty where free
  const uint32_t* slot_rank;           // the record of the key beside it
  unsigned long long mask;             // slots - 1, slots a power of two
  uint32_t max_probe;
  float inv;                           // 1.0f / resolution
  const float* mean3;
  const double* creg6;
};

// the first slot of a key: a 64-bit finalizer (every input bit reaches every output bit), so that keys that differ only
// in z, or only above bit 32, spread over a small table
__device__ __forceinline__ unsigned long long vg_mix(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

struct VgSums {  // a run's nine chains
  double x, y, z, xx, xy, xz, yy, yz, zz;
};
__device__ __forceinline__ void vg_first(VgSums& a, float fx, float fy, float fz) {  // assigned, not added to zero
  const double x = double(fx), y = double(fy), z = double(fz);
  a.x = x; a.y = y; a.z = z;
  a.xx = x * x; a.xy = x * y; a.xz = x * z; a.yy = y * y; a.yz = y * z; a.zz = z * z;
}
__device__ __forceinline__ void vg_add(VgSums& a, float fx, float fy, float fz) {
  const double x = double(fx), y = double(fy), z = double(fz);
  a.x += x; a.y += y; a.z += z;
  a.xx += x * x; a.xy += x * y; a.xz += x * z; a.yy += y * y; a.yz += y * z; a.zz += z * z;
}

// voxel_distribution_map.hpp:231-256: the record of run [i0, end) into slot r
__device__ __forceinline__ void vg_emit(const VgSums& a, unsigned i0, unsigned end, unsigned r,
                                        const unsigned long long* __restrict__ keys, double eps, const VgRecords& O,
                                        VgStat* __restrict__ stat) {
  const uint32_t count = end - i0;
  const double cnt = double(count);
  const double mx = a.x / cnt, my = a.y / cnt, mz = a.z / cnt;
  O.key[r] = keys[i0];
  O.count[r] = count;
  float* const m = O.mean3 + size_t(r) * 3;
  m[0] = float(mx); m[1] = float(my); m[2] = float(mz);
  float* const c = O.cov9 + size_t(r) * 9;
  double* const g = O.creg6 + size_t(r) * 6;
  if (count >= 3u) {  // E[X XT] - E[X] E[X]T in double, no contraction, stored as float
    const float cxx = float(__dsub_rn(a.xx / cnt, __dmul_rn(mx, mx)));
    const float cxy = float(__dsub_rn(a.xy / cnt, __dmul_rn(mx, my)));
    const float cxz = float(__dsub_rn(a.xz / cnt, __dmul_rn(mx, mz)));
    const float cyy = float(__dsub_rn(a.yy / cnt, __dmul_rn(my, my)));
    const float cyz = float(__dsub_rn(a.yz / cnt, __dmul_rn(my, mz)));
    const float czz = float(__dsub_rn(a.zz / cnt, __dmul_rn(mz, mz)));
    const float cf[9] = {cxx, cxy, cxz, cxy, cyy, cyz, cxz, cyz, czz};
#pragma unroll
    for (int q = 0; q < 9; ++q) c[q] = cf[q];
    reg_regularize_one(cf, eps, g);
  } else {            // float(eps) I, and no preferred direction
    const float e = float(eps);
#pragma unroll
    for (int q = 0; q < 9; ++q) c[q] = (q == 0 || q == 4 || q == 8) ? e : 0.0f;
    g[0] = 1.0; g[1] = 0.0; g[2] = 0.0; g[3] = 1.0; g[4] = 0.0; g[5] = 1.0;
    atomicAdd(&stat->n_sparse, 1u);
  }
  atomicMax(&stat->max_count, count);
}

// One lane per run.  x, y, z: the valid points in sorted order (k_vx_heads' stage); pos: n_out + 1 run starts.
inline __global__ __launch_bounds__(256) void k_vg_reduce(unsigned n_out, const uint32_t* __restrict__ pos,
                                                          const unsigned long long* __restrict__ keys,
                                                          const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ z, double eps, const VgRecords O,
                                                          VgStat* __restrict__ stat, uint32_t* __restrict__ long_list) {
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_out) return;
  const unsigned i0 = pos[r], end = pos[r + 1u];
  if (end - i0 > kVxLong) {
    long_list[atomicAdd(&stat->long_count, 1u)] = r;
    return;
  }
  VgSums a;
  vg_first(a, x[i0], y[i0], z[i0]);
  for (unsigned j = i0 + 1u; j < end; j += kVgBatch) {
    float vx[kVgBatch], vy[kVgBatch], vz[kVgBatch];
#pragma unroll
    for (unsigned u = 0; u < kVgBatch; ++u) {
      const unsigned q = min(j + u, end - 1u);
      vx[u] = x[q]; vy[u] = y[q]; vz[u] = z[q];
    }
#pragma unroll
    for (unsigned u = 0; u < kVgBatch; ++u)
      if (j + u < end) vg_add(a, vx[u], vy[u], vz[u]);
  }
  vg_emit(a, i0, end, r, keys, eps, O, stat);
}

// One wavefront per long run (grid-stride over the list): 64 consecutive entries per load, one per lane, every lane
// adding them up in order (lane k's values by readlane), the next 64 already on their way.
inline __global__ __launch_bounds__(64) void k_vg_reduce_long(const uint32_t* __restrict__ long_list,
                                                              const uint32_t* __restrict__ pos,
                                                              const unsigned long long* __restrict__ keys,
                                                              const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ z, double eps, const VgRecords O,
                                                              VgStat* __restrict__ stat) {
  const unsigned lane = threadIdx.x;
  const unsigned n_long = stat->long_count;
  for (unsigned q = blockIdx.x; q < n_long; q += gridDim.x) {
    const unsigned r = long_list[q];
    const unsigned i0 = pos[r], end = pos[r + 1u];
    VgSums a;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (i0 + lane < end) { cx = x[i0 + lane]; cy = y[i0 + lane]; cz = z[i0 + lane]; }
    vg_first(a, vx_lane(cx, 0u), vx_lane(cy, 0u), vx_lane(cz, 0u));
    for (unsigned base = i0; base < end; base += 64u) {
      const unsigned nj = base + 64u + lane;
      float nx = 0.0f, ny = 0.0f, nz = 0.0f;
      if (nj < end) { nx = x[nj]; ny = y[nj]; nz = z[nj]; }
      const unsigned m = min(64u, end - base);
      for (unsigned k = base == i0 ? 1u : 0u; k < m; ++k) vg_add(a, vx_lane(cx, k), vx_lane(cy, k), vx_lane(cz, k));
      cx = nx; cy = ny; cz = nz;
    }
    if (lane == 0u) vg_emit(a, i0, end, r, keys, eps, O, stat);
  }
}

// One lane per voxel.  slot_key: `mask + 1` entries, all kVgEmpty before the launch; the table is at most half full, so
// an insertion ends within mask + 1 probes.
inline __global__ __launch_bounds__(256) void k_vg_insert(unsigned num_voxels, const unsigned long long* __restrict__ key,
                                                          unsigned long long* __restrict__ slot_key,
                                                          uint32_t* __restrict__ slot_rank, unsigned long long mask,
                                                          VgStat* __restrict__ stat) {
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  if (r >= num_voxels) return;
  const unsigned long long k = key[r];
  const unsigned long long h = vg_mix(k);
  for (unsigned long long p = 0; p <= mask; ++p) {
    const unsigned long long s = (h + p) & mask;
    if (atomicCAS(&slot_key[s], kVgEmpty, k) == kVgEmpty) {
      slot_rank[s] = r;
      atomicMax(&stat->max_probe, uint32_t(min(p + 1ull, 0xFFFFFFFFull)));
      return;
    }
  }
}

// whether key k has a voxel, and its rank: at most M.max_probe slots from the key's first
__device__ __forceinline__ bool vg_lookup(const VgTable& M, unsigned long long k, uint32_t& rank) {
  const unsigned long long h = vg_mix(k);
  for (uint32_t p = 0; p < M.max_probe; ++p) {
    const unsigned long long s = (h + p) & M.mask;
    const unsigned long long at = M.slot_key[s];
    if (at == k) {
      rank = M.slot_rank[s];
      return true;
    }
    if (at == kVgEmpty) return false;
  }
  return false;
}

// corr (nullable): corr[i] = the rank of the voxel source point i falls into, -1 for none
inline __global__ __launch_bounds__(kRegThreads) void k_vg_linearize(unsigned n, const float* __restrict__ sx,
                                                                     const float* __restrict__ sy,
                                                                     const float* __restrict__ sz,
                                                                     const double* __restrict__ s_creg,
                                                                     const RegTransform T, const VgTable M, int kernel,
                                                                     double width, double* __restrict__ partial,
                                                                     int32_t* __restrict__ corr) {
  const unsigned i = blockIdx.x * unsigned(kRegThreads) + threadIdx.x;
  double S[kRegSums];
#pragma unroll
  for (int a = 0; a < kRegSums; ++a) S[a] = 0.0;
  if (i < n) {
    double px, py, pz;
    reg_transform(T, double(sx[i]), double(sy[i]), double(sz[i]), px, py, pz);
    // the voxel of p cast to float (voxel_correspondence.hpp:61); the factor takes the double
    uint32_t j = 0u;
    const bool hit = vg_lookup(M, voxel_pack(float(px), float(py), float(pz), M.inv), j);
    if (hit) {
      const float* const m = M.mean3 + size_t(j) * 3;
      double Cs[6], Ct[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        Cs[a] = s_creg[size_t(i) * 6 + size_t(a)];
        Ct[a] = M.creg6[size_t(j) * 6 + size_t(a)];
      }
      reg_factor_gicp(px, py, pz, double(m[0]), double(m[1]), double(m[2]), T.r, Cs, Ct, kernel, width, S);
      S[28] = 1.0;
    }
    if (corr) corr[i] = hit ? int32_t(j) : -1;
  }
  reg_block_sum(S, partial);
}

}  // namespace fdm
