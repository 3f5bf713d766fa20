// fdm_pcd.hpp — binary PCD records <-> SoA channels on the device.  gfx950 only.
//
// Reference being reproduced: fastdem/lib/nanoPCL/include/nanopcl/io/pcd_io.hpp — readFieldAsFloat :209-230 and the
// binary branch of loadPCD :332-375 (k_pcd_decode), the binary branch of savePCD :516-545 (k_pcd_pack).  Unlike the
// PointCloud2 ingest (fdm_ingest.hpp) no point is dropped: output index == record index, NaN and infinite coordinates
// included.
//
// k_pcd_decode: a block takes 256 consecutive records, one contiguous slab of 256 * point_size bytes.  Records of up to
// kPcdLdsMaxPoint bytes are staged through LDS — 16-byte loads when the body's base is 16-byte aligned (256 * point_size
// is a multiple of 16, so every slab then starts aligned), 4-byte loads when it is 4-byte aligned, single bytes
// otherwise (a body that is a slice of a larger device buffer starts anywhere) — and each lane then picks its record's
// fields out of LDS.  Lane l reads at l * point_size + offset: with a point_size of 16 or 32 bytes that stride would put
// a 32-lane half on 8 or 4 of the 32 banks a 4-byte LDS read sees, so the slab is stored with one padding word behind
// every 32 (byte a at a + 4 * (a / 128)): strides of 4 and 8 words then spread over all 32 banks, odd word strides
// (12-, 20-byte records) stay conflict-free.  Fields that are not 4-byte aligned inside the slab (13-, 19-byte
// records) are put together from single-byte LDS reads.  Larger records are read straight from memory, field by field.
// LDS budget: 256 * 128 B * 33 / 32 = 33 792 B per block, four blocks per CU within 160 KiB and below the 64 KiB a
// launch gets without asking.
//
// k_pcd_pack: each lane loads its point's channels (coalesced per channel), the block's records are put together in LDS
// (the same padding: a record stride of 4 or 8 words would otherwise serialise the writes) and leave as one contiguous
// run of 4-byte stores, 256 bytes per wavefront instruction.
#pragma once

#include "fdm_device.hpp"

namespace fdm {

constexpr unsigned kPcdBlockPoints = 256;
constexpr unsigned kPcdLdsMaxPoint = 128;   // largest point_size the LDS path takes
constexpr unsigned kPcdMaxPoint = 1024;     // largest point_size at all
constexpr unsigned kPcdLdsWords = kPcdBlockPoints * kPcdLdsMaxPoint / 4u;
constexpr unsigned kPcdLdsPadded = kPcdLdsWords + kPcdLdsWords / 32u;

// how readFieldAsFloat treats a field: its (type, size) pair
enum PcdKind : int { PCD_ZERO = 0, PCD_F4 = 1, PCD_F8 = 2, PCD_U1 = 3, PCD_U4 = 4, PCD_I4 = 5 };

struct PcdDecode {
  unsigned point_size;
  int stage;        // LDS path: bytes per staging load (16, 4 or 1); 0 = the direct path
  int aligned;      // every chosen 4- / 8-byte field sits on a 4-byte boundary (of LDS, or of memory on the direct path)
  int off[8];       // x, y, z, intensity, rgb, nx, ny, nz: byte offset in the record
  int kind[8];      // PcdKind (rgb: unused)
  void* out[8];     // null = not wanted
};

__device__ __forceinline__ unsigned pcd_pad(unsigned a) { return a + ((a >> 7) << 2); }  // byte address in the padded slab

struct PcdLdsSrc {
  const uint8_t* s;  // padded slab
  __device__ __forceinline__ uint32_t byte(unsigned a) const { return s[pcd_pad(a)]; }
  __device__ __forceinline__ uint32_t word(unsigned a) const { return *reinterpret_cast<const uint32_t*>(s + pcd_pad(a)); }
};
struct PcdMemSrc {
  const uint8_t* s;
  __device__ __forceinline__ uint32_t byte(size_t a) const { return s[a]; }
  __device__ __forceinline__ uint32_t word(size_t a) const { return *reinterpret_cast<const uint32_t*>(s + a); }
};

template <typename Src, typename Addr>
__device__ __forceinline__ uint32_t pcd_u32(const Src& S, Addr a, bool aligned) {
  if (aligned) return S.word(a);
  return S.byte(a) | (S.byte(a + 1) << 8) | (S.byte(a + 2) << 16) | (S.byte(a + 3) << 24);
}

template <typename Src, typename Addr>
__device__ __forceinline__ float pcd_field(const Src& S, Addr a, int kind, bool aligned) {
  switch (kind) {
    case PCD_F4: return __uint_as_float(pcd_u32(S, a, aligned));
    case PCD_F8: {
      const unsigned long long lo = pcd_u32(S, a, aligned), hi = pcd_u32(S, a + 4, aligned);
      return static_cast<float>(__longlong_as_double((long long)(lo | (hi << 32))));
    }
    case PCD_U1: return float(S.byte(a));
    case PCD_U4: return float(pcd_u32(S, a, aligned));
    case PCD_I4: return float(int(pcd_u32(S, a, aligned)));
    default: return 0.0f;
  }
}

template <typename Src, typename Addr>
__device__ __forceinline__ void pcd_emit(const Src& S, Addr rec, const PcdDecode& D, unsigned long long i) {
  const bool al = D.aligned != 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (!D.out[k]) continue;
    if (k == 4)  // the four bytes at the colour field, whatever its declared type: 0x00RRGGBB
      static_cast<uint32_t*>(D.out[4])[i] = pcd_u32(S, rec + Addr(D.off[4]), al) & 0x00FFFFFFu;
    else
      static_cast<float*>(D.out[k])[i] = pcd_field(S, rec + Addr(D.off[k]), D.kind[k], al);
  }
}

// n records of D.point_size bytes at `body` (at least n * point_size bytes) -> the wanted channels
inline __global__ __launch_bounds__(256) void k_pcd_decode(const uint8_t* __restrict__ body, const PcdDecode D,
                                                    unsigned long long n) {
  __shared__ uint32_t s_slab[kPcdLdsPadded];
  const unsigned long long first = (unsigned long long)blockIdx.x * kPcdBlockPoints;
  const unsigned long long i = first + threadIdx.x;
  if (D.stage == 0) {
    if (i < n) pcd_emit(PcdMemSrc{body}, size_t(i) * D.point_size, D, i);
    return;
  }
  const unsigned long long left = n - first;
  const unsigned in_block = left < kPcdBlockPoints ? unsigned(left) : kPcdBlockPoints;
  const unsigned bytes = in_block * D.point_size;  // <= 32 768
  const uint8_t* const src = body + size_t(first) * D.point_size;
  uint8_t* const s8 = reinterpret_cast<uint8_t*>(s_slab);
  unsigned done = 0;  // bytes the wide loads cover
  if (D.stage == 16) {
    done = bytes & ~15u;
    for (unsigned a = threadIdx.x * 16u; a < done; a += 256u * 16u) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + a);
      uint32_t* const d = reinterpret_cast<uint32_t*>(s8 + pcd_pad(a));  // 16 bytes never cross a 128-byte boundary
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else if (D.stage == 4) {
    done = bytes & ~3u;
    for (unsigned a = threadIdx.x * 4u; a < done; a += 256u * 4u)
      *reinterpret_cast<uint32_t*>(s8 + pcd_pad(a)) = *reinterpret_cast<const uint32_t*>(src + a);
  }
  for (unsigned a = done + threadIdx.x; a < bytes; a += 256u) s8[pcd_pad(a)] = src[a];
  __syncthreads();
  if (i < n) pcd_emit(PcdLdsSrc{s8}, threadIdx.x * D.point_size, D, i);
}

struct PcdPack {
  int n_words;            // words per record: 3 .. 8
  const void* ch[8];      // x, y, z, intensity, rgb, nx, ny, nz: null = absent (the normals: all three or none)
};

// n points -> n records of P.n_words words at `out`, in savePCD's field order
inline __global__ __launch_bounds__(256) void k_pcd_pack(const PcdPack P, unsigned long long n, uint32_t* __restrict__ out) {
  __shared__ uint32_t s_rec[256 * 8 + 256 * 8 / 32];
  const unsigned long long first = (unsigned long long)blockIdx.x * 256u;
  const unsigned long long i = first + threadIdx.x;
  if (i < n) {
    unsigned w = threadIdx.x * unsigned(P.n_words);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (!P.ch[k]) continue;
      uint32_t v = static_cast<const uint32_t*>(P.ch[k])[i];
      if (k == 4) v &= 0x00FFFFFFu;  // r << 16 | g << 8 | b
      s_rec[w + (w >> 5)] = v;
      ++w;
    }
  }
  __syncthreads();
  const unsigned long long left = n - first;
  const unsigned words = (left < 256u ? unsigned(left) : 256u) * unsigned(P.n_words);
  uint32_t* const dst = out + size_t(first) * size_t(P.n_words);
  for (unsigned w = threadIdx.x; w < words; w += 256u) dst[w] = s_rec[w + (w >> 5)];
}

}  // namespace fdm
