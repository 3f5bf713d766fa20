// fdm_render.hpp — one map layer -> an RGBA8 colour image on the device (fastdem::io::savePng's pixels).  gfx950 only.
//
// Reference being reproduced: fastdem/src/io_png.cpp:32-65 (computeRange) and :67-171 (the three colour functions and
// savePng's pixel loop).  The reference gathers the finite cells on the host and runs two std::nth_element; here the two
// order statistics come out of ONE radix select over monotone 32-bit keys (ord(), fdm_device.hpp): four 8-bit digit
// passes over the layer, each a 256-bin histogram per block in LDS merged into one global table, with a one-block
// kernel in between that picks the bin of BOTH ranks and narrows both key prefixes.  The finite count n — and with it
// the two ranks, in fp64 as the reference computes them — falls out of the first pass, min / max ride in it too, so
// nothing returns to the host before the image does.  The colour kernel reads the column-major layer and writes
// row-major pixels through a padded LDS tile: both sides are coalesced.
#pragma once

#include "fdm_device.hpp"

namespace fdm {

enum { kNormMinMax = 0, kNormPercentile = 1, kNormFixed = 2 };
enum { kMapGray = 0, kMapViridis = 1, kMapJet = 2 };

// Zero-initialised (hipMemsetAsync) at the start of every render.
struct RenderState {
  unsigned hist[2][256];  // the current pass's digit counts among the keys under prefix[q]; k_render_pick clears them
  unsigned n;             // finite cells
  unsigned not_min_key;   // max over ~ord(v), so that zero is the identity of both extremes
  unsigned max_key;
  unsigned rank[2];       // rank still to go inside prefix[q]
  unsigned prefix[2];     // the digits chosen so far, in place (low bits zero)
  float range[2];         // the result: {min, max} of the normalisation
};

struct RenderParams {
  int s_rows, s_cols;  // the stored window: image height, width
  int stride;          // floats between consecutive cells of the layer (1, or the record size)
  int slot;            // geometry ring slot
  int use_start;       // 1: unroll the circular buffer from the start index (align_to_world on an untiled engine)
  int normalize, colormap;
  float fixed_min, fixed_max;
};

// One wavefront's keys into the block's LDS table.  A layer's values usually share sign and exponent, so in the first
// pass whole wavefronts agree on the digit: 64 atomics on one LDS word would take 64 LDS cycles, one lane adds the
// count instead.
__device__ __forceinline__ void render_hist_add(unsigned* h, bool take, unsigned digit) {
  const unsigned long long act = __ballot(take);
  if (act == 0ull) return;
  const int leader = __ffsll((long long)act) - 1;
  const unsigned d0 = unsigned(__shfl(int(digit), leader));
  const unsigned long long same = __ballot(take && digit == d0);
  if (same == act) {
    if (int(threadIdx.x & 63u) == leader) atomicAdd(&h[d0], unsigned(__popcll(act)));
  } else if (take) {
    atomicAdd(&h[digit], 1u);
  }
}

// Digit pass PASS (0: bits 31-24 ... 3: bits 7-0) over the finite cells.  Pass 0 also counts them and takes min / max.
template <int PASS>
__global__ __launch_bounds__(256) void k_render_hist(const float* __restrict__ layer, int stride, unsigned ncell,
                                                     RenderState* __restrict__ rs) {
  __shared__ unsigned s_h[2][256];
  __shared__ unsigned s_ext[2];
  constexpr int shift = 24 - 8 * PASS;
  s_h[0][threadIdx.x] = 0u;
  s_h[1][threadIdx.x] = 0u;
  if (threadIdx.x < 2) s_ext[threadIdx.x] = 0u;
  unsigned p0 = 0u, p1 = 0u;
  if (PASS > 0) { p0 = rs->prefix[0]; p1 = rs->prefix[1]; }
  const bool split = p0 != p1;  // the two ranks have parted: two tables
  __syncthreads();
  unsigned not_mn = 0u, mx = 0u;
  const unsigned step = gridDim.x * 256u;
  for (unsigned base = blockIdx.x * 256u; base < ncell; base += step) {  // (block-uniform trip count: the ballots are whole)
    const unsigned i = base + threadIdx.x;
    const bool in = i < ncell;
    const float v = in ? layer[size_t(i) * size_t(stride)] : NAN;
    const bool fin = in && isfinite(v);
    const unsigned key = ord(v);
    const unsigned digit = (key >> shift) & 255u;
    if (PASS == 0) {
      render_hist_add(s_h[0], fin, digit);
      if (fin) { not_mn = max(not_mn, ~key); mx = max(mx, key); }
    } else {
      const unsigned hi = (key >> shift) >> 8;  // the digits above this one
      render_hist_add(s_h[0], fin && hi == ((p0 >> shift) >> 8), digit);
      if (split) render_hist_add(s_h[1], fin && hi == ((p1 >> shift) >> 8), digit);
    }
  }
  if (PASS == 0) {
    if (not_mn) atomicMax(&s_ext[0], not_mn);  // (a finite key is never 0xFFFFFFFF nor 0: those are NaN patterns)
    if (mx) atomicMax(&s_ext[1], mx);
  }
  __syncthreads();
  const unsigned c0 = s_h[0][threadIdx.x];
  if (c0) atomicAdd(&rs->hist[0][threadIdx.x], c0);
  if (PASS > 0) {
    const unsigned c1 = s_h[1][threadIdx.x];
    if (c1) atomicAdd(&rs->hist[1][threadIdx.x], c1);
  }
  if (PASS == 0 && threadIdx.x < 2 && s_ext[threadIdx.x])
    atomicMax(threadIdx.x == 0 ? &rs->not_min_key : &rs->max_key, s_ext[threadIdx.x]);
}

// One block between the passes: n and the two ranks (after pass 0), then for each rank the bin that holds it.
// computeRange (io_png.cpp:57-59): idx_1 = size_t(n * 0.01), idx_99 = min(size_t(n * 0.99), n - 1), products in double.
template <int PASS>
__global__ __launch_bounds__(256) void k_render_pick(RenderState* __restrict__ rs, int normalize) {
  __shared__ unsigned s_wave[2][4];
  __shared__ unsigned s_rank[2], s_pre[2];
  constexpr int shift = 24 - 8 * PASS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool split = PASS > 0 && rs->prefix[0] != rs->prefix[1];
  unsigned h[2], incl[2];
  h[0] = rs->hist[0][threadIdx.x];
  h[1] = split ? rs->hist[1][threadIdx.x] : h[0];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    unsigned s = h[q];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(s, d);
      if (lane >= d) s += o;
    }
    incl[q] = s;
    if (lane == 63) s_wave[q][w] = s;
  }
  if (threadIdx.x < 2) { s_rank[threadIdx.x] = rs->rank[threadIdx.x]; s_pre[threadIdx.x] = rs->prefix[threadIdx.x]; }
  __syncthreads();
  const unsigned n = PASS == 0 ? s_wave[0][0] + s_wave[0][1] + s_wave[0][2] + s_wave[0][3] : rs->n;
  if (PASS == 0 && threadIdx.x == 0) {
    rs->n = n;
    if (n) {
      const unsigned long long k1 = (unsigned long long)(double(n) * 0.01);
      const unsigned long long k99 = (unsigned long long)(double(n) * 0.99);
      s_rank[0] = unsigned(k1);
      s_rank[1] = unsigned(k99 < (unsigned long long)(n - 1u) ? k99 : (unsigned long long)(n - 1u));
    }
  }
  __syncthreads();
  rs->hist[0][threadIdx.x] = 0u;  // (every read of the tables is behind the barriers above)
  rs->hist[1][threadIdx.x] = 0u;
  if (n == 0u) {
    if (threadIdx.x == 0) { rs->range[0] = 0.0f; rs->range[1] = 1.0f; }  // io_png.cpp:49-51
    return;
  }
  if (normalize == kNormMinMax) {
    if (threadIdx.x == 0) { rs->range[0] = unord(~rs->not_min_key); rs->range[1] = unord(rs->max_key); }
    return;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    unsigned before = incl[q] - h[q];
    for (int k = 0; k < w; ++k) before += s_wave[q][k];
    const unsigned r = s_rank[q];
    if (h[q] && before <= r && r < before + h[q]) {  // exactly one bin: the rank is below the count under the prefix
      const unsigned pre = s_pre[q] | (threadIdx.x << shift);
      rs->rank[q] = r - before;
      rs->prefix[q] = pre;
      if (PASS == 3) rs->range[q] = unord(pre);
    }
  }
}

// ---- colour (io_png.cpp:67-113) ----
__device__ __forceinline__ unsigned render_u8(float x) { return unsigned(static_cast<unsigned char>(x)); }
__device__ __forceinline__ float render_clamp01(float t) {  // std::max(0.0f, std::min(1.0f, t))
  const float a = (t < 1.0f) ? t : 1.0f;
  return (0.0f < a) ? a : 0.0f;
}

__device__ __forceinline__ unsigned render_pixel(float v, float vmin, float range, int colormap) {
  // the eight control colours of the reference's viridis table (the contract, like the config defaults)
  constexpr float kViridis[8][3] = {{0.267f, 0.005f, 0.329f}, {0.283f, 0.141f, 0.458f}, {0.254f, 0.265f, 0.530f},
                                    {0.207f, 0.372f, 0.553f}, {0.164f, 0.471f, 0.558f}, {0.128f, 0.567f, 0.551f},
                                    {0.267f, 0.679f, 0.481f}, {0.993f, 0.906f, 0.144f}};
  if (!isfinite(v)) return 0u;  // RGBA 0, 0, 0, 0
  const float t = render_clamp01((v - vmin) / range);
  unsigned r, g, b;
  if (colormap == kMapViridis) {
    const float idx = t * 7.0f;
    const int i0 = static_cast<int>(idx);
    const int i1 = min(i0 + 1, 7);
    const float frac = idx - static_cast<float>(i0);
    const float keep = 1.0f - frac;
    r = render_u8((kViridis[i0][0] * keep + kViridis[i1][0] * frac) * 255.0f + 0.5f);
    g = render_u8((kViridis[i0][1] * keep + kViridis[i1][1] * frac) * 255.0f + 0.5f);
    b = render_u8((kViridis[i0][2] * keep + kViridis[i1][2] * frac) * 255.0f + 0.5f);
  } else if (colormap == kMapJet) {
    if (t < 0.25f) {
      r = 0u; g = render_u8(4.0f * t * 255.0f + 0.5f); b = 255u;
    } else if (t < 0.5f) {
      r = 0u; g = 255u; b = render_u8((1.0f - 4.0f * (t - 0.25f)) * 255.0f + 0.5f);
    } else if (t < 0.75f) {
      r = render_u8(4.0f * (t - 0.5f) * 255.0f + 0.5f); g = 255u; b = 0u;
    } else {
      r = 255u; g = render_u8((1.0f - 4.0f * (t - 0.75f)) * 255.0f + 0.5f); b = 0u;
    }
  } else {
    r = g = b = render_u8(t * 255.0f + 0.5f);
  }
  return r | (g << 8) | (b << 16) | 0xFF000000u;  // bytes R, G, B, A in memory
}

// One 64 x 64-pixel tile per block.  In: lanes run down a buffer column (consecutive layer memory but for the one wrap
// of the circular buffer); out: lanes run along an image row.  The tile's LDS rows are 65 words, so the column-wise
// writes and the row-wise reads both touch 64 different banks.
constexpr int kRenderTile = 64;
inline __global__ __launch_bounds__(256) void k_render_colour(const RenderParams Q, const float* __restrict__ layer,
                                                              const DevState* __restrict__ st,
                                                              const RenderState* __restrict__ rs,
                                                              uint32_t* __restrict__ out) {
  __shared__ uint32_t s_px[kRenderTile][kRenderTile + 1];  // [image column][image row]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = int(blockIdx.y) * kRenderTile, c0 = int(blockIdx.x) * kRenderTile;
  int sr = 0, sc = 0;
  if (Q.use_start) { sr = st->geom[Q.slot].sr; sc = st->geom[Q.slot].sc; }
  float vmin = Q.fixed_min, vmax = Q.fixed_max;
  if (Q.normalize != kNormFixed) { vmin = rs->range[0]; vmax = rs->range[1]; }
  float range = vmax - vmin;
  if (range < 1e-6f) range = 1.0f;
  const int r = r0 + lane;
  int br = r + sr;  // (r + start_row) % rows
  br -= br >= Q.s_rows ? Q.s_rows : 0;
  for (int k = w; k < kRenderTile; k += 4) {
    const int c = c0 + k;
    if (r < Q.s_rows && c < Q.s_cols) {
      int bc = c + sc;
      bc -= bc >= Q.s_cols ? Q.s_cols : 0;
      const float v = layer[(size_t(bc) * size_t(Q.s_rows) + size_t(br)) * size_t(Q.stride)];
      s_px[k][lane] = render_pixel(v, vmin, range, Q.colormap);
    }
  }
  __syncthreads();
  const int oc = c0 + lane;
  for (int k = w; k < kRenderTile; k += 4) {
    const int orow = r0 + k;
    if (orow < Q.s_rows && oc < Q.s_cols) out[size_t(orow) * size_t(Q.s_cols) + size_t(oc)] = s_px[lane][k];
  }
}

}  // namespace fdm
