// fdm_dem.hpp — the per-cell histogram filter of buildDEM and the order-keeping compaction between its stages.  gfx950.
//
// Reference being reproduced: fastdem/src/pcd_convert.cpp:194-269 (findGroundPeak, removeFloatingPoints).  Per map cell:
// a histogram of the cell's z values over bins of `bin` metres from the cell's z_min; the LOWEST bin with the largest
// count is the ground peak; a point stays iff z <= (z_min + (best_bin + 0.5f) * bin) + height_threshold.  The number of
// bins is unbounded ((z_max - z_min) / bin), the number of non-empty bins is not: no histogram is allocated.
//   k_ras_ids (fdm_raster.hpp)  cell id per point (`ncell` = the reference skips the point)
//   k_hf_minmax  per-cell z_min / z_max: ordered-key atomics (min and max do not depend on the order)
//   k_hf_bins    per point: bin = min(int((z - z_min) / bin), n_bins - 1); flags a cell whose bin count leaves int32
//   fdm_rsort    stable sort by bin, then by cell: a cell's points are one run, its bins ascending runs inside it
//   k_hf_peak    the lane at the head of a cell's run finds the FIRST longest run of equal bins, stores the cutoff
//   k_hf_keep    per point, in input order: z <= cutoff of its cell
#pragma once

#include "fdm_device.hpp"

namespace fdm {

struct DemStat {
  uint32_t bad;      // some cell's (z_max - z_min) / bin does not fit an int32 (or is not a number)
  uint32_t max_bin;  // largest bin index of any point: the bits the first sort needs
  uint32_t n_kept;
  uint32_t pad;
};

inline __global__ void k_dem_stat_init(DemStat* __restrict__ st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) st->bad = st->max_bin = st->n_kept = st->pad = 0u;
}

// cmin / cmax: ord(z), initialised to 0xFFFFFFFF / 0
inline __global__ __launch_bounds__(256) void k_hf_minmax(unsigned n, const uint32_t* __restrict__ cell,
                                                          const float* __restrict__ z, uint32_t ncell,
                                                          uint32_t* __restrict__ cmin, uint32_t* __restrict__ cmax) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cell[i];
  if (c >= ncell) return;
  const uint32_t o = ord(z[i]);
  atomicMin(&cmin[c], o);
  atomicMax(&cmax[c], o);
}

inline __global__ __launch_bounds__(256) void k_hf_bins(unsigned n, const uint32_t* __restrict__ cell,
                                                        const float* __restrict__ z, uint32_t ncell,
                                                        const uint32_t* __restrict__ cmin,
                                                        const uint32_t* __restrict__ cmax, float bin,
                                                        uint32_t* __restrict__ bins, DemStat* __restrict__ st) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  uint32_t b = 0u;
  bool bad = false;
  if (i < n) {
    const uint32_t c = cell[i];
    if (c < ncell) {
      const float z_min = unord(cmin[c]), z_max = unord(cmax[c]);
      const float span = __fdiv_rn(__fsub_rn(z_max, z_min), bin);
      if (!(span < 2147483648.0f) || !(span >= 0.0f)) bad = true;  // static_cast<int> of it is undefined: refused
      else {
        const int n_bins = max(1, int(span) + 1);                  // :200 (span <= 2147483520: no overflow)
        b = uint32_t(min(int(__fdiv_rn(__fsub_rn(z[i], z_min), bin)), n_bins - 1));  // :204
      }
    }
    bins[i] = b;
  }
  uint32_t m = b;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) m = max(m, uint32_t(__shfl_xor(int(m), s)));
  const unsigned long long mb = __ballot(bad);
  if ((threadIdx.x & 63u) == 0u) {
    if (m) atomicMax(&st->max_bin, m);
    if (mb) atomicOr(&st->bad, 1u);
  }
}

// out[q] = src[idx[q]]
inline __global__ __launch_bounds__(256) void k_dem_gather_u32(unsigned n, const uint32_t* __restrict__ idx,
                                                               const uint32_t* __restrict__ src,
                                                               uint32_t* __restrict__ out) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q < n) out[q] = src[idx[q]];
}

// keys / idx: the pairs sorted by (cell, bin, index).  cutoff[cell] (float bits) is written by the head of the cell's run.
inline __global__ __launch_bounds__(256) void k_hf_peak(unsigned n, const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ idx, uint32_t ncell,
                                                        const uint32_t* __restrict__ bins,
                                                        const uint32_t* __restrict__ cmin, float bin,
                                                        float height_threshold, uint32_t* __restrict__ cutoff) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n) return;
  const uint32_t c = keys[p];
  if (c >= ncell || (p != 0u && keys[p - 1u] == c)) return;
  uint32_t cur = bins[idx[p]], best_bin = cur;
  unsigned cur_count = 0u, best_count = 0u;
#pragma unroll 1
  for (unsigned q = p; q < n && keys[q] == c; ++q) {
    const uint32_t b = bins[idx[q]];
    if (b != cur) { cur = b; cur_count = 0u; }
    ++cur_count;
    if (cur_count > best_count) { best_count = cur_count; best_bin = cur; }  // strict: the lowest bin wins a tie (:213)
  }
  const float z_min = unord(cmin[c]);
  const float ground = __fadd_rn(z_min, __fmul_rn(__fadd_rn(float(int(best_bin)), 0.5f), bin));  // :219
  cutoff[c] = __float_as_uint(__fadd_rn(ground, height_threshold));                              // :257
}

inline __global__ __launch_bounds__(256) void k_hf_keep(unsigned n, const uint32_t* __restrict__ cell,
                                                        const float* __restrict__ z, uint32_t ncell,
                                                        const uint32_t* __restrict__ cutoff,
                                                        uint8_t* __restrict__ keep, DemStat* __restrict__ st) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  bool in = false;
  if (i < n) {
    const uint32_t c = cell[i];
    in = c < ncell && z[i] <= __uint_as_float(cutoff[c]);  // :260
    keep[i] = in ? 1 : 0;
  }
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&st->n_kept, unsigned(__popcll(m)));
}

// ---- compaction in input order (nanopcl::filters::filter / PointCloud::extract): counts per block of 256, k_pack_scan
// (fdm_egress.hpp) over them, then every kept point moves to offsets[block] + its rank inside the block ----
inline __global__ __launch_bounds__(256) void k_dem_count(unsigned n, const uint8_t* __restrict__ keep,
                                                          uint32_t* __restrict__ counts) {
  __shared__ unsigned s_w[4];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned long long m = __ballot(i < n && keep[i] != 0);
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = unsigned(__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0u) counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

struct DemChannels {
  const float* in[5];  // x, y, z, intensity, rgb (as 32-bit words); nullptr = no such channel
  float* out[5];
};
inline __global__ __launch_bounds__(256) void k_dem_compact(unsigned n, const uint8_t* __restrict__ keep,
                                                            const uint32_t* __restrict__ offsets, const DemChannels C) {
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
  const size_t d = size_t(offsets[blockIdx.x]) + rank;
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (C.in[k]) C.out[k][d] = C.in[k][i];
}

}  // namespace fdm
