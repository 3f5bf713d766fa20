// fdm_introsort.hpp — the order libstdc++'s std::sort leaves on the voxel filter's (key, point index) pairs, on the
// device (option "voxel_any_order" = 1, fdm_engine_ray.inl).  gfx950 only.
//
// Reference being served: lib/nanoPCL/include/nanopcl/filters/impl/voxel_grid_impl.hpp:46-63,171-172 — VoxelMode::ANY
// takes idx[start + (count*7 + start*13) % count] after an UNSTABLE std::sort on the key alone, so which point of a
// voxel represents it is whatever libstdc++'s introsort leaves.  The restatement the kernels rest on (checked against
// std::sort by scripts/introsort_model.py and tests/test_voxel_order_model.py):
//   * the array is the valid points only, in point order (a stable compaction drops the non-finite ones first);
//     depth limit 2 * floor(log2 n); ranges of more than 16 elements are partitioned while depth is left;
//   * a partition step on [f, l): the median of f+1, f+(l-f)/2, l-1 (libstdc++'s branch order) is swapped into f, its
//     key is the pivot p; of [f+1, l), the positions with key >= p counted from the left (g_1 < g_2 < ...) pair with
//     those with key <= p counted from the right (r_1 > r_2 > ...).  Pair k swaps iff g_k < r_k (a prefix of K
//     pairs); the cut is min(g_{K+1}, r_K), or g_1 if K = 0; both children go on with one depth less;
//   * a range of more than 16 elements with no depth left ends as make_heap + sort_heap leave it (is_heap_sort);
//   * the final insertion pass never crosses a partition boundary, so every leaf of <= 16 elements ends stably sorted.
// Pipeline (one stream, no host round trip; the launch count is fixed by n on the host):
//   compaction   k_is_ccount -> k_is_cscan (also seeds the segment lists) -> k_is_cscatter: valid pairs in point
//                order into buf[0]; dropped points (invalid key) behind position nv of the output, as the radix
//                sort leaves them
//   levels       per level, over every segment of more than kIsLds elements (tiles of kIsTile elements):
//                k_is_plan (median to first, tiles) -> k_is_count (>= / <= per tile) -> k_is_scan (segmented
//                offsets) -> k_is_pos (rank -> position tables) -> k_is_scatter (K by a 64-way search, the swaps,
//                out of place; elements of children that leave the level passes go straight to the output)
//   finish       k_is_finish: one wavefront per segment of <= kIsLds elements, in LDS: the remaining levels, the
//                heap fallback, the stable leaves.  k_is_rest: segments still larger than kIsLds after the last level
//                (or at depth 0), one wavefront each, the same routine on global memory.
// Worst case of k_is_rest: only adversarial inputs reach it (a median-of-3 killer): one wavefront runs the rest of the
// introsort of a range of m elements, about m * depth / 64 dependent global round trips plus, at the depth limit, a
// heap sort by one lane (m log2 m dependent loads) — seconds for a multi-million-point range.  Evidence that real
// scans do not get there is synthetic only: the tests' random, sorted and tie-heavy clouds and the synthetic VLP-16,
// RGB-D and LiDAR-128 scans (its kernel-trace time on those is that of a launch with no segment); it has not been
// checked on recorded sensor data.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace fdm {

constexpr unsigned kIsLds = 2048u;   // segments up to this size finish in one wavefront's LDS (k_is_finish)
constexpr unsigned kIsTile = 4096u;  // elements per block of the level passes (256 threads x 16)
constexpr unsigned kIsLeaf = 16u;    // libstdc++'s _S_threshold

struct IsSeg {
  unsigned f, l;  // [f, l) of the array
  int depth;      // depth left
  int src;        // k_is_finish: 1 = the elements are still in buf[0] (the whole array was small), 0 = in the output
};
struct IsCtl {
  unsigned nv;        // valid points
  unsigned nbig[2];   // segments of the level passes, by level parity
  unsigned nfin;      // segments for k_is_finish
  unsigned nrest;     // segments for k_is_rest
  unsigned ntiles;    // tiles of the current level
  unsigned pad[2];
};
template <typename KEY>
struct IsBufs {
  KEY* key[2];          // level buffers (key[0] / idx[0]: the compaction's output)
  uint32_t* idx[2];
  KEY* okey;            // output: vkeys[1] / vidx[1]
  uint32_t* oidx;
  uint32_t* posg;       // [f + rank]: position of the rank-th element >= pivot from the left
  uint32_t* posr;       // [f + rank]: position of the rank-th element <= pivot from the right
  IsSeg* big[2];        // level segments, by level parity (cap_big each)
  IsSeg* fin;           // cap_fin
  IsSeg* rest;          // cap_big
  KEY* piv;             // per level segment: pivot key
  uint32_t* tile0;      // per level segment: first tile
  uint32_t* tot;        // per level segment: elements >= / <= pivot (2 words)
  uint32_t* tile_seg;   // per tile: segment
  uint32_t* tile_cnt;   // per tile: >= | <= << 16 (compaction: valid points)
  uint32_t* tile_ag;    // per tile: >= of all earlier tiles (compaction: valid points of the earlier tiles)
  uint32_t* tile_ar;    // per tile: <= of this and all earlier tiles
  uint32_t* tile_og;    // per tile: >= of the segment's earlier tiles
  uint32_t* tile_or;    // per tile: <= of the segment's later tiles
  IsCtl* ctl;
  unsigned cap_big, cap_fin, cap_tiles;
};

template <typename KEY>
struct IsInvalid;
template <>
struct IsInvalid<unsigned long long> {
  static constexpr unsigned long long v = ~0ull;
};
template <>
struct IsInvalid<uint32_t> {
  static constexpr uint32_t v = 0xFFFFFFFFu;
};

__host__ __device__ inline int is_depth_limit(unsigned n) {  // 2 * std::__lg(n)
  int lg = 0;
  while ((n >> lg) > 1u) ++lg;
  return 2 * lg;
}

// exclusive prefix of v over a block of 256 threads (4 wavefronts); *total = the block's sum
__device__ __forceinline__ uint32_t is_block_excl(uint32_t v, uint32_t* s_w, uint32_t* total) {
  const unsigned t = threadIdx.x, lane = t & 63u, w = t >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (int(lane) >= d) x += y;
  }
  if (lane == 63u) s_w[w] = x;
  __syncthreads();
  uint32_t base = 0u;
  for (unsigned k = 0; k < w; ++k) base += s_w[k];
  *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  __syncthreads();
  return base + x - v;
}

// ---- compaction: valid pairs in point order ----
template <typename KEY>
__global__ __launch_bounds__(256) void k_is_ccount(unsigned n, const KEY* __restrict__ keys, IsBufs<KEY> B) {
  __shared__ uint32_t s_w[4];
  const unsigned b = blockIdx.x * kIsTile + threadIdx.x * 16u;
  uint32_t c = 0u;
  for (unsigned j = 0; j < 16u; ++j)
    if (b + j < n && keys[b + j] != IsInvalid<KEY>::v) ++c;
  uint32_t total;
  is_block_excl(c, s_w, &total);
  if (threadIdx.x == 0) B.tile_cnt[blockIdx.x] = total;
}

// one block: exclusive prefix of the tiles' valid counts; nv; the first segment
template <typename KEY>
__global__ __launch_bounds__(256) void k_is_cscan(unsigned ntiles, IsBufs<KEY> B) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0u;
  __syncthreads();
  for (unsigned c0 = 0; c0 < ntiles; c0 += 256u) {
    const unsigned t = c0 + threadIdx.x;
    const uint32_t v = t < ntiles ? B.tile_cnt[t] : 0u;
    uint32_t total;
    const uint32_t ex = is_block_excl(v, s_w, &total);
    if (t < ntiles) B.tile_ag[t] = s_carry + ex;
    __syncthreads();
    if (threadIdx.x == 0) s_carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    IsCtl& c = *B.ctl;
    const unsigned nv = s_carry;
    c.nv = nv;
    c.nbig[0] = c.nbig[1] = 0u;
    c.nfin = c.nrest = c.ntiles = 0u;
    const IsSeg s{0u, nv, is_depth_limit(nv), 1};
    if (nv > kIsLds) { B.big[0][0] = s; c.nbig[0] = 1u; }
    else if (nv > 0u) { B.fin[0] = s; c.nfin = 1u; }
  }
}

template <typename KEY>
__global__ __launch_bounds__(256) void k_is_cscatter(unsigned n, const KEY* __restrict__ keys, IsBufs<KEY> B) {
  __shared__ uint32_t s_w[4];
  const unsigned b = blockIdx.x * kIsTile + threadIdx.x * 16u;
  KEY k[16];
  uint32_t c = 0u, m = 0u;
#pragma unroll
  for (unsigned j = 0; j < 16u; ++j) {
    k[j] = b + j < n ? keys[b + j] : IsInvalid<KEY>::v;
    if (b + j < n && k[j] != IsInvalid<KEY>::v) { ++c; m |= 1u << j; }
  }
  uint32_t total;
  unsigned v = B.tile_ag[blockIdx.x] + is_block_excl(c, s_w, &total);  // valid points before b
  const unsigned nv = B.ctl->nv;
#pragma unroll
  for (unsigned j = 0; j < 16u; ++j) {
    const unsigned i = b + j;
    if (i >= n) break;
    if (m >> j & 1u) {
      B.key[0][v] = k[j];
      B.idx[0][v] = i;
      ++v;
    } else {  // dropped: behind every valid point, in point order
      B.okey[nv + (i - v)] = IsInvalid<KEY>::v;
      B.oidx[nv + (i - v)] = i;
    }
  }
}

// ---- level passes ----
// one block: median of three to first, pivot, tiles of every segment of this level
template <typename KEY>
__global__ __launch_bounds__(256) void k_is_plan(int level, IsBufs<KEY> B) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_carry;
  const int cur = level & 1;
  IsCtl& c = *B.ctl;
  const unsigned S = c.nbig[cur];
  KEY* const key = B.key[cur];
  uint32_t* const idx = B.idx[cur];
  if (threadIdx.x == 0) s_carry = 0u;
  __syncthreads();
  for (unsigned c0 = 0; c0 < S; c0 += 256u) {
    const unsigned s = c0 + threadIdx.x;
    uint32_t tiles = 0u;
    if (s < S) {
      const IsSeg g = B.big[cur][s];
      const unsigned f = g.f, l = g.l;
      const unsigned a = f + 1u, bm = f + (l - f) / 2u, cc = l - 1u;
      const KEY ka = key[a], kb = key[bm], kc = key[cc];
      unsigned m;  // __move_median_to_first
      if (ka < kb) m = kb < kc ? bm : (ka < kc ? cc : a);
      else if (ka < kc) m = a;
      else m = kb < kc ? cc : bm;
      const KEY kf = key[f], km = key[m];
      const uint32_t xf = idx[f], xm = idx[m];
      key[f] = km; idx[f] = xm;
      key[m] = kf; idx[m] = xf;
      B.piv[s] = km;
      tiles = (l - f - 1u + kIsTile - 1u) / kIsTile;
    }
    uint32_t total;
    const uint32_t ex = is_block_excl(tiles, s_w, &total);
    if (s < S) {
      const unsigned t0 = s_carry + ex;
      B.tile0[s] = t0;
      for (unsigned t = 0; t < tiles; ++t) B.tile_seg[t0 + t] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    c.ntiles = s_carry;
    c.nbig[cur ^ 1] = 0u;
  }
}

// the tile's elements, >= / <= pivot flags of its 16 per thread
template <typename KEY>
struct IsTileView {
  unsigned s, f, l, b, e, j;  // segment, its range, the tile [b, e), tile index inside the segment
  KEY p;
};
template <typename KEY>
__device__ __forceinline__ bool is_tile(const IsBufs<KEY>& B, int cur, IsTileView<KEY>& T) {
  if (blockIdx.x >= B.ctl->ntiles) return false;
  T.s = B.tile_seg[blockIdx.x];
  const IsSeg g = B.big[cur][T.s];
  T.f = g.f;
  T.l = g.l;
  T.j = blockIdx.x - B.tile0[T.s];
  T.b = g.f + 1u + T.j * kIsTile;
  T.e = min(T.b + kIsTile, g.l);
  T.p = B.piv[T.s];
  return true;
}
template <typename KEY>
__device__ __forceinline__ void is_classify(const KEY* __restrict__ key, const IsTileView<KEY>& T, uint32_t& ge,
                                            uint32_t& le) {
  ge = le = 0u;
  const unsigned b = T.b + threadIdx.x * 16u;
#pragma unroll
  for (unsigned j = 0; j < 16u; ++j) {
    if (b + j < T.e) {
      const KEY k = key[b + j];
      if (!(k < T.p)) ge |= 1u << j;
      if (!(T.p < k)) le |= 1u << j;
    }
  }
}

template <typename KEY>
__global__ __launch_bounds__(256) void k_is_count(int level, IsBufs<KEY> B) {
  __shared__ uint32_t s_w[4];
  IsTileView<KEY> T;
  if (!is_tile(B, level & 1, T)) return;
  uint32_t ge, le;
  is_classify(B.key[level & 1], T, ge, le);
  uint32_t total;
  is_block_excl(uint32_t(__popc(ge)) | (uint32_t(__popc(le)) << 16), s_w, &total);
  if (threadIdx.x == 0) B.tile_cnt[blockIdx.x] = total;
}

// one block: per tile, the >= of the segment's earlier tiles and the <= of its later ones; per segment, the totals
template <typename KEY>
__global__ __launch_bounds__(256) void k_is_scan(int level, IsBufs<KEY> B) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_carry_g, s_carry_r;
  const IsCtl& c = *B.ctl;
  const unsigned nt = c.ntiles, S = c.nbig[level & 1];
  // pass 1: over ALL tiles (a segment's tiles are a contiguous run): exclusive >= prefix, inclusive <= prefix
  if (threadIdx.x == 0) { s_carry_g = 0u; s_carry_r = 0u; }
  __syncthreads();
  for (unsigned c0 = 0; c0 < nt; c0 += 256u) {
    const unsigned t = c0 + threadIdx.x;
    const uint32_t v = t < nt ? B.tile_cnt[t] : 0u;
    uint32_t tg, tr;
    const uint32_t eg = is_block_excl(v & 0xFFFFu, s_w, &tg);
    const uint32_t er = is_block_excl(v >> 16, s_w, &tr);
    if (t < nt) {
      B.tile_ag[t] = s_carry_g + eg;
      B.tile_ar[t] = s_carry_r + er + (v >> 16);
    }
    __syncthreads();
    if (threadIdx.x == 0) { s_carry_g += tg; s_carry_r += tr; }
    __syncthreads();
  }
  // pass 2: per segment, its totals; per tile, the counts rebased to its segment
  for (unsigned s = threadIdx.x; s < S; s += 256u) {
    const unsigned t0 = B.tile0[s], t1 = s + 1u < S ? B.tile0[s + 1u] : nt;
    const uint32_t g1 = t1 < nt ? B.tile_ag[t1] : s_carry_g;
    B.tot[2u * s] = g1 - B.tile_ag[t0];
    B.tot[2u * s + 1u] = B.tile_ar[t1 - 1u] - (B.tile_ar[t0] - (B.tile_cnt[t0] >> 16));
  }
  for (unsigned t = threadIdx.x; t < nt; t += 256u) {
    const unsigned s = B.tile_seg[t], t0 = B.tile0[s];
    const unsigned t1 = s + 1u < S ? B.tile0[s + 1u] : nt;
    B.tile_og[t] = B.tile_ag[t] - B.tile_ag[t0];     // >= in the segment's earlier tiles
    B.tile_or[t] = B.tile_ar[t1 - 1u] - B.tile_ar[t];  // <= in its later tiles
  }
}

// the tile's ranks: ge rank from the left (segment-wide), le rank from the right; fills the rank -> position tables
template <typename KEY>
__device__ __forceinline__ void is_ranks(const IsBufs<KEY>& B, uint32_t ge, uint32_t le,
                                         uint32_t* s_w, uint32_t& rg, uint32_t& rr) {
  uint32_t total;
  const uint32_t ex = is_block_excl(uint32_t(__popc(ge)) | (uint32_t(__popc(le)) << 16), s_w, &total);
  // rg: >= elements before this thread's first one (segment-wide); rr: <= elements after this thread's last one
  rg = B.tile_og[blockIdx.x] + (ex & 0xFFFFu);
  rr = B.tile_or[blockIdx.x] + ((total >> 16) - (ex >> 16) - uint32_t(__popc(le)));
}

template <typename KEY>
__global__ __launch_bounds__(256) void k_is_pos(int level, IsBufs<KEY> B) {
  __shared__ uint32_t s_w[4];
  IsTileView<KEY> T;
  if (!is_tile(B, level & 1, T)) return;
  uint32_t ge, le, rg, rr;
  is_classify(B.key[level & 1], T, ge, le);
  is_ranks(B, ge, le, s_w, rg, rr);
  const unsigned b = T.b + threadIdx.x * 16u;
  uint32_t rr_hi = rr + uint32_t(__popc(le));  // walking left to right, the <= rank from the right counts down
#pragma unroll
  for (unsigned j = 0; j < 16u; ++j) {
    if (ge >> j & 1u) B.posg[T.f + rg++] = b + j;
    if (le >> j & 1u) B.posr[T.f + --rr_hi] = b + j;
  }
}

// K (swapped pairs) of segment s: the number of ranks a with posg[f + a] < posr[f + a] (a prefix), 64-way search by
// one wavefront
__device__ __forceinline__ unsigned is_search_k(const uint32_t* __restrict__ pg, const uint32_t* __restrict__ pr,
                                                unsigned hi) {
  const unsigned lane = threadIdx.x & 63u;
  unsigned lo = 0u;
  while (lo < hi) {
    const unsigned step = (hi - lo + 63u) / 64u;
    const unsigned a = lo + lane * step;
    const bool t = a < hi && pg[a] < pr[a];
    const unsigned c = unsigned(__popcll(__ballot(t)));
    if (c == 0u) { hi = lo; break; }
    const unsigned nlo = lo + (c - 1u) * step + 1u, nhi = min(lo + c * step, hi);
    lo = nlo;
    hi = nhi;
  }
  return lo;
}

template <typename KEY>
__global__ __launch_bounds__(256) void k_is_scatter(int level, int last, IsBufs<KEY> B) {
  __shared__ uint32_t s_w[4];
  __shared__ unsigned s_k;
  IsTileView<KEY> T;
  const int cur = level & 1;
  if (!is_tile(B, cur, T)) return;
  const unsigned cg = B.tot[2u * T.s], cr = B.tot[2u * T.s + 1u];
  const uint32_t* pg = B.posg + T.f;
  const uint32_t* pr = B.posr + T.f;
  if (threadIdx.x < 64u) {
    const unsigned k = is_search_k(pg, pr, min(cg, cr));
    if (threadIdx.x == 0) s_k = k;
  }
  __syncthreads();
  const unsigned K = s_k;
  const unsigned cut = K == 0u ? pg[0] : (K < cg ? min(pg[K], pr[K - 1u]) : pr[K - 1u]);
  const int d = B.big[cur][T.s].depth - 1;
  // where the elements of a child go: on through the level passes, or to the output (k_is_finish / k_is_rest)
  const auto stays = [&](unsigned f, unsigned l) { return l - f > kIsLds && d > 0 && !last; };
  const bool left_on = stays(T.f, cut), right_on = stays(cut, T.l);
  KEY* const nk = B.key[cur ^ 1];
  uint32_t* const ni = B.idx[cur ^ 1];
  const KEY* const key = B.key[cur];
  const uint32_t* const idx = B.idx[cur];
  uint32_t ge, le, rg, rr;
  is_classify(key, T, ge, le);
  is_ranks(B, ge, le, s_w, rg, rr);
  const unsigned b = T.b + threadIdx.x * 16u;
  uint32_t rr_hi = rr + uint32_t(__popc(le));
#pragma unroll
  for (unsigned j = 0; j < 16u; ++j) {
    const unsigned i = b + j;
    unsigned dst = i;
    if (ge >> j & 1u) { if (rg < K) dst = pr[rg]; ++rg; }
    if (le >> j & 1u) { --rr_hi; if (rr_hi < K) dst = pg[rr_hi]; }
    if (i < T.e) {
      const bool on = dst < cut ? left_on : right_on;
      (on ? nk : B.okey)[dst] = key[i];
      (on ? ni : B.oidx)[dst] = idx[i];
    }
  }
  if (T.j == 0u && threadIdx.x == 0) {
    (left_on ? nk : B.okey)[T.f] = key[T.f];  // the pivot stays at f
    (left_on ? ni : B.oidx)[T.f] = idx[T.f];
    IsCtl& c = *B.ctl;
    const unsigned ends[3] = {T.f, cut, T.l};
    for (int h = 0; h < 2; ++h) {
      const unsigned f = ends[h], l = ends[h + 1];
      if (l - f < 2u) continue;
      const IsSeg s{f, l, d, 0};
      if (stays(f, l)) B.big[cur ^ 1][atomicAdd(&c.nbig[cur ^ 1], 1u)] = s;
      else if (l - f > kIsLds) B.rest[atomicAdd(&c.nrest, 1u)] = s;
      else B.fin[atomicAdd(&c.nfin, 1u)] = s;
    }
  }
}

// ---- the rest of the introsort of one range, by one wavefront (blockDim 64) ----
// __adjust_heap followed by __push_heap, on k / ix [0, n)
template <typename KEY>
__device__ void is_adjust_heap(KEY* k, uint32_t* ix, long long hole, long long n, KEY vk, uint32_t vi) {
  const long long top = hole;
  long long child = hole;
  while (child < (n - 1) / 2) {
    child = 2 * (child + 1);
    if (k[child] < k[child - 1]) --child;
    k[hole] = k[child];
    ix[hole] = ix[child];
    hole = child;
  }
  if ((n & 1) == 0 && child == (n - 2) / 2) {
    child = 2 * (child + 1);
    k[hole] = k[child - 1];
    ix[hole] = ix[child - 1];
    hole = child - 1;
  }
  long long parent = (hole - 1) / 2;
  while (hole > top && k[parent] < vk) {
    k[hole] = k[parent];
    ix[hole] = ix[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  k[hole] = vk;
  ix[hole] = vi;
}
// __partial_sort(first, last, last) = __make_heap + __sort_heap; one lane
template <typename KEY>
__device__ void is_heap_sort(KEY* k, uint32_t* ix, long long n) {
  if (n < 2) return;
  for (long long parent = (n - 2) / 2;; --parent) {
    is_adjust_heap(k, ix, parent, n, k[parent], ix[parent]);
    if (parent == 0) break;
  }
  while (n > 1) {
    --n;
    const KEY vk = k[n];
    const uint32_t vi = ix[n];
    k[n] = k[0];
    ix[n] = ix[0];
    is_adjust_heap(k, ix, 0, n, vk, vi);
  }
}

// [0, m) of k / ix at depth d0, to the end of std::sort; pg / pr: m entries of scratch each; stk: 3 * 72 words of LDS
template <typename KEY, typename POS>
__device__ void is_wave_sort(KEY* k, uint32_t* ix, POS* pg, POS* pr, unsigned m, int d0, unsigned* stk) {
  const unsigned lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  if (m < 2u) return;
  if (lane == 0) { stk[0] = 0u; stk[1] = m; stk[2] = unsigned(d0); }
  int sp = 1;
  __syncthreads();
  while (sp > 0) {
    --sp;
    unsigned f = stk[3 * sp], l = stk[3 * sp + 1];
    int d = int(stk[3 * sp + 2]);
    __syncthreads();
    bool heaped = false;
    while (l - f > kIsLeaf) {
      if (d == 0) {
        if (lane == 0) is_heap_sort(k + f, ix + f, (long long)(l - f));
        __syncthreads();
        heaped = true;
        break;
      }
      --d;
      if (lane == 0) {
        const unsigned a = f + 1u, bm = f + (l - f) / 2u, cc = l - 1u;
        const KEY ka = k[a], kb = k[bm], kc = k[cc];
        unsigned mm;
        if (ka < kb) mm = kb < kc ? bm : (ka < kc ? cc : a);
        else if (ka < kc) mm = a;
        else mm = kb < kc ? cc : bm;
        const KEY kf = k[f], km = k[mm];
        const uint32_t xf = ix[f], xm = ix[mm];
        k[f] = km; ix[f] = xm;
        k[mm] = kf; ix[mm] = xf;
      }
      __syncthreads();
      const KEY p = k[f];
      unsigned cg = 0u, cr = 0u;
      for (unsigned b = f + 1u; b < l; b += 64u) {
        const unsigned i = b + lane;
        const bool ge = i < l && !(k[i] < p);
        const unsigned long long mk = __ballot(ge);
        if (ge) pg[cg + unsigned(__popcll(mk & below))] = POS(i);
        cg += unsigned(__popcll(mk));
      }
      for (int top = int(l) - 1; top >= int(f) + 1; top -= 64) {
        const int i = top - int(lane);
        const bool le = i >= int(f) + 1 && !(p < k[i]);
        const unsigned long long mk = __ballot(le);
        if (le) pr[cr + unsigned(__popcll(mk & below))] = POS(i);
        cr += unsigned(__popcll(mk));
      }
      __syncthreads();
      const unsigned mn = min(cg, cr);
      unsigned K = 0u;
      for (unsigned a0 = 0; a0 < mn; a0 += 64u) {
        const unsigned a = a0 + lane;
        const unsigned c = unsigned(__popcll(__ballot(a < mn && unsigned(pg[a]) < unsigned(pr[a]))));
        K += c;
        if (c != 64u) break;
      }
      for (unsigned a = lane; a < K; a += 64u) {  // disjoint pairs: every g_a < every r_b of the swapped ones
        const unsigned x = pg[a], y = pr[a];
        const KEY kx = k[x], ky = k[y];
        const uint32_t ixx = ix[x], ixy = ix[y];
        k[x] = ky; ix[x] = ixy;
        k[y] = kx; ix[y] = ixx;
      }
      const unsigned cut = K == 0u ? unsigned(pg[0]) : (K < cg ? min(unsigned(pg[K]), unsigned(pr[K - 1u])) : unsigned(pr[K - 1u]));
      __syncthreads();
      if (lane == 0) { stk[3 * sp] = cut; stk[3 * sp + 1] = l; stk[3 * sp + 2] = unsigned(d); }
      ++sp;
      l = cut;
      __syncthreads();
    }
    if (!heaped && l - f >= 2u) {  // a leaf: what the insertion pass leaves is its stable order
      const unsigned len = l - f;
      KEY kv{};
      uint32_t iv = 0u;
      unsigned r = 0u;
      if (lane < len) {
        kv = k[f + lane];
        iv = ix[f + lane];
        for (unsigned j = 0; j < len; ++j) {
          const KEY kj = k[f + j];
          r += (kj < kv || (kj == kv && j < lane)) ? 1u : 0u;
        }
      }
      __syncthreads();
      if (lane < len) { k[f + r] = kv; ix[f + r] = iv; }
      __syncthreads();
    }
  }
}

template <typename KEY>
__global__ __launch_bounds__(64) void k_is_finish(IsBufs<KEY> B) {
  __shared__ KEY s_k[kIsLds];
  __shared__ uint32_t s_i[kIsLds];
  __shared__ uint16_t s_g[kIsLds], s_r[kIsLds];
  __shared__ unsigned s_stk[3 * 72];
  const unsigned nfin = B.ctl->nfin;
  for (unsigned q = blockIdx.x; q < nfin; q += gridDim.x) {
    const IsSeg g = B.fin[q];
    const unsigned m = g.l - g.f;
    const KEY* sk = g.src ? B.key[0] : B.okey;
    const uint32_t* si = g.src ? B.idx[0] : B.oidx;
    for (unsigned i = threadIdx.x; i < m; i += 64u) { s_k[i] = sk[g.f + i]; s_i[i] = si[g.f + i]; }
    __syncthreads();
    is_wave_sort<KEY, uint16_t>(s_k, s_i, s_g, s_r, m, g.depth, s_stk);
    __syncthreads();
    for (unsigned i = threadIdx.x; i < m; i += 64u) { B.okey[g.f + i] = s_k[i]; B.oidx[g.f + i] = s_i[i]; }
    __syncthreads();
  }
}

template <typename KEY>
__global__ __launch_bounds__(64) void k_is_rest(IsBufs<KEY> B) {
  __shared__ unsigned s_stk[3 * 72];
  const unsigned nrest = B.ctl->nrest;
  for (unsigned q = blockIdx.x; q < nrest; q += gridDim.x) {
    const IsSeg g = B.rest[q];
    is_wave_sort<KEY, uint32_t>(B.okey + g.f, B.oidx + g.f, B.posg + g.f, B.posr + g.f, g.l - g.f, g.depth, s_stk);
    __syncthreads();
  }
}

}  // namespace fdm
