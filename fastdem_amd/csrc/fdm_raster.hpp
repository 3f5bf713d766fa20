// fdm_raster.hpp — a static point cloud into the map, and the map back into a cloud, on the device.  gfx950 only.
//
// Reference being reproduced: fastdem/src/pcd_convert.cpp:29-185 (fromPointCloud, both overloads) and :327-373
// (toPointCloud).  No sensor model, no poses, no estimator: per cell the reference runs Welford's update in fp32 over
// the cell's points IN INPUT ORDER (BatchCellStats::addZ), and mean / m2 depend on that order in their last bits and
// sometimes beyond.  So no float atomics and no tree reduction here:
//   k_ras_ids    per point: linear cell id from the fp64 getIndex arithmetic (cell_of, circular start index included),
//                or `ncell` for a point the reference skips (NaN z, getIndex false) — a key that sorts behind every cell
//   fdm_rsort    stable LSD radix sort of (cell id, point index) over the bits of `ncell`: ties stay in point order
//   k_ras_walk   one lane per touched cell (the lane at the head of the cell's run) applies the run's points one after
//                another — Welford, min, max, first-or-greater intensity, last colour — and writes the cell ONCE
// min / max / intensity / colour ride the same walk (they could be ordered-key atomics as in k_bin; one walk is simpler
// and the points are already in hand).  Untouched cells are never written.
#pragma once

#include "fdm_device.hpp"

namespace fdm {

// device words both directions share (fdm_engine::pc_stat)
struct RasterStat {
  uint32_t n_used;         // points that landed in a cell
  uint32_t n_cells;        // cells written
  uint32_t has_int;        // toPointCloud: some emitted cell has a non-NaN intensity / colour
  uint32_t has_col;
  uint32_t min_x, min_y;   // ord() of the cloud's bounding box over points whose x and y are both non-NaN
  uint32_t max_x, max_y;
};

inline __global__ void k_ras_stat_init(RasterStat* __restrict__ st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->n_used = st->n_cells = st->has_int = st->has_col = 0u;
    st->min_x = st->min_y = ord(kFltMax);    // std::numeric_limits<float>::max() / lowest(): pcd_convert.cpp:160-163
    st->max_x = st->max_y = ord(-kFltMax);
  }
}

// pcd_convert.cpp:165-172.  (Of +0 and -0 the reference keeps whichever came first; here -0 is the smaller one.  The
// sums and differences the geometry is made of do not tell them apart, except that a box of zeros only may give the
// position -0.0 where the reference has +0.0.)
inline __global__ __launch_bounds__(256) void k_ras_bounds(unsigned n, const float* __restrict__ x,
                                                           const float* __restrict__ y, RasterStat* __restrict__ st) {
  float mnx = kFltMax, mny = kFltMax, mxx = -kFltMax, mxy = -kFltMax;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const float px = x[i], py = y[i];
    if (px != px || py != py) continue;
    mnx = px < mnx ? px : mnx; mny = py < mny ? py : mny;
    mxx = px > mxx ? px : mxx; mxy = py > mxy ? py : mxy;
  }
  uint32_t a = ord(mnx), b = ord(mny), c = ord(mxx), d = ord(mxy);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    a = min(a, uint32_t(__shfl_xor(int(a), s)));
    b = min(b, uint32_t(__shfl_xor(int(b), s)));
    c = max(c, uint32_t(__shfl_xor(int(c), s)));
    d = max(d, uint32_t(__shfl_xor(int(d), s)));
  }
  if ((threadIdx.x & 63u) == 0u) {
    atomicMin(&st->min_x, a); atomicMin(&st->min_y, b);
    atomicMax(&st->max_x, c); atomicMax(&st->max_y, d);
  }
}

// keys[i] = col * rows + row of point i, or ncell (dropped): pcd_convert.cpp:74-80
inline __global__ __launch_bounds__(256) void k_ras_ids(unsigned n, const float* __restrict__ x,
                                                        const float* __restrict__ y, const float* __restrict__ z,
                                                        const GeomConst G, const DevState* __restrict__ state, int slot,
                                                        uint32_t ncell, uint32_t* __restrict__ keys,
                                                        RasterStat* __restrict__ st) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  bool in = false;
  if (i < n) {
    const DevGeom g = state->geom[slot];
    DevCand cand;
    cand.px = g.px; cand.py = g.py; cand.sr = g.sr; cand.sc = g.sc; cand.shr = cand.shc = 0;
    const float pz = z[i];
    int r = 0, c = 0;
    in = !(pz != pz) && cell_of(x[i], y[i], cand, G, r, c);
    keys[i] = in ? uint32_t(c) * uint32_t(G.rows) + uint32_t(r) : ncell;
  }
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&st->n_used, unsigned(__popcll(m)));
}

enum { kRasElev = 0, kRasMin, kRasMax, kRasVar, kRasCount, kRasIntensity, kRasColor, kRasLayers };
struct RasterLayers {
  float* p[kRasLayers];  // element 0 of the layer (own array or record field); intensity / colour: nullptr = no channel
  int s[kRasLayers];     // distance between cells, in floats
};

// keys / idx: the sorted pairs.  Lane p owns the cell whose run starts at p.
inline __global__ __launch_bounds__(256) void k_ras_walk(unsigned n, const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ idx, uint32_t ncell,
                                                         const float* __restrict__ z,
                                                         const float* __restrict__ intensity,
                                                         const uint32_t* __restrict__ rgb, int method,
                                                         const RasterLayers L, RasterStat* __restrict__ st) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  bool head = false;
  uint32_t k = ncell;
  if (p < n) {
    k = keys[p];
    head = k < ncell && (p == 0u || keys[p - 1u] != k);
  }
  if (head) {
    // BatchCellStats (pcd_convert.cpp:32-59)
    float mean = 0.0f, m2 = 0.0f, min_z = kFltMax, max_z = -kFltMax, max_int = -kFltMax;
    uint32_t count = 0u, color = 0u;
    bool has_int = false;
    for (unsigned q = p; q < n && keys[q] == k; ++q) {
      const uint32_t i = idx[q];
      const float v = z[i];
      ++count;
      const float delta = v - mean;
      mean += delta / float(count);
      const float delta2 = v - mean;
      m2 += delta * delta2;
      if (v < min_z) min_z = v;
      if (v > max_z) max_z = v;
      if (intensity) {
        const float a = intensity[i];
        if (!has_int || a > max_int) { max_int = a; has_int = true; }
      }
      if (rgb) color = rgb[i] & 0x00FFFFFFu;
    }
    const size_t o = k;
    const float elev = method == 1 ? min_z : (method == 2 ? mean : max_z);  // Max, Min, Mean, MinMax (:125-138)
    L.p[kRasElev][o * size_t(L.s[kRasElev])] = elev;
    L.p[kRasMin][o * size_t(L.s[kRasMin])] = min_z;
    L.p[kRasMax][o * size_t(L.s[kRasMax])] = max_z;
    L.p[kRasVar][o * size_t(L.s[kRasVar])] = count < 2u ? 0.0f : m2 / float(count - 1u);
    L.p[kRasCount][o * size_t(L.s[kRasCount])] = float(count);
    if (intensity) L.p[kRasIntensity][o * size_t(L.s[kRasIntensity])] = max_int;
    if (rgb) reinterpret_cast<uint32_t*>(L.p[kRasColor])[o * size_t(L.s[kRasColor])] = color;
  }
  const unsigned long long m = __ballot(head);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&st->n_cells, unsigned(__popcll(m)));
}

// ---- toPointCloud (pcd_convert.cpp:327-373) ----
// ASSUMED (nanoGrid's map.cells() is not on disk): the visiting order fdm_engine_pack_cloud uses for the whole map —
// unwrapped column by unwrapped column from the start index, rows fastest (fdm_egress.hpp pack_cell).  Visit t is the
// unwrapped cell (t % rows, t / rows).
struct CloudLayers {
  const float* elev; int elev_stride;
  const float* intensity; int int_stride;  // nullptr: the map has no such layer
  const float* color;
};
struct CloudCell {
  bool valid, has_int, has_col;
  int ur, uc;
  float z, intensity;
  uint32_t rgb;
};
__device__ __forceinline__ CloudCell cloud_cell(const GeomConst& G, const DevGeom& g, const CloudLayers& L,
                                                unsigned long long t, unsigned long long total) {
  CloudCell cc;
  cc.valid = cc.has_int = cc.has_col = false;
  cc.ur = cc.uc = 0;
  cc.z = cc.intensity = 0.f;
  cc.rgb = 0u;
  if (t >= total) return cc;
  cc.uc = int(t / unsigned(G.rows));
  cc.ur = int(t - (unsigned long long)cc.uc * unsigned(G.rows));
  int r = g.sr + cc.ur, c = g.sc + cc.uc;
  r -= r >= G.rows ? G.rows : 0;
  c -= c >= G.cols ? G.cols : 0;
  const size_t o = size_t(c) * G.rows + r;
  cc.z = L.elev[o * size_t(L.elev_stride)];
  cc.valid = !(cc.z != cc.z);  // std::isnan only: an infinite elevation is a point
  if (!cc.valid) return cc;
  if (L.intensity) {
    const float a = L.intensity[o * size_t(L.int_stride)];
    if (!(a != a)) { cc.has_int = true; cc.intensity = a; }
  }
  if (L.color) {
    const float packed = L.color[o];
    if (!(packed != packed)) { cc.has_col = true; cc.rgb = __float_as_uint(packed) & 0x00FFFFFFu; }
  }
  return cc;
}

inline __global__ __launch_bounds__(256) void k_cloud_count(const GeomConst G, const DevState* __restrict__ state,
                                                            int slot, const CloudLayers L,
                                                            uint32_t* __restrict__ counts, RasterStat* __restrict__ st) {
  __shared__ unsigned s_w[4];
  const DevGeom g = state->geom[slot];
  const unsigned long long t = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  const CloudCell cc = cloud_cell(G, g, L, t, (unsigned long long)G.rows * G.cols);
  const unsigned long long m = __ballot(cc.valid), mi = __ballot(cc.has_int), mc = __ballot(cc.has_col);
  if ((threadIdx.x & 63) == 0) {
    s_w[threadIdx.x >> 6] = unsigned(__popcll(m));
    if (mi) atomicOr(&st->has_int, 1u);
    if (mc) atomicOr(&st->has_col, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// offsets: the exclusive scan of k_cloud_count's block counts (k_pack_scan); out: x | y | z | intensity | rgb, `cap` each
inline __global__ __launch_bounds__(256) void k_cloud_write(const GeomConst G, const DevState* __restrict__ state,
                                                            int slot, const CloudLayers L,
                                                            const uint32_t* __restrict__ offsets,
                                                            float* __restrict__ out, size_t cap) {
  __shared__ unsigned s_w[4];
  const DevGeom g = state->geom[slot];
  const unsigned long long t = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  const CloudCell cc = cloud_cell(G, g, L, t, (unsigned long long)G.rows * G.cols);
  const unsigned long long m = __ballot(cc.valid);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_w[w] = unsigned(__popcll(m));
  __syncthreads();
  if (!cc.valid) return;
  unsigned rank = unsigned(__popcll(m & ((1ull << lane) - 1ull)));
  for (int q = 0; q < w; ++q) rank += s_w[q];
  const size_t d = size_t(offsets[blockIdx.x]) + rank;
  if (d >= cap) return;
  const double origin_x = g.px + G.len_x / 2.0 - G.res / 2.0;
  const double origin_y = g.py + G.len_y / 2.0 - G.res / 2.0;
  out[d] = static_cast<float>(origin_x - double(cc.ur) * G.res);
  out[cap + d] = static_cast<float>(origin_y - double(cc.uc) * G.res);
  out[2 * cap + d] = cc.z;
  out[3 * cap + d] = cc.intensity;  // 0 where the cell has none (a default-constructed channel entry)
  reinterpret_cast<uint32_t*>(out)[4 * cap + d] = cc.rgb;
}

}  // namespace fdm
