// fdm_engine_pcd.inl — host side of the PCD file codec (nanopcl/io/pcd_io.hpp: loadPCD :243-378, savePCD :415-550) and of
// the pcd2dem tool's two calls (fastdem/tools/pcd2dem.cpp).  Part of fdm_engine_post.hip, behind fdm_engine_cloud.inl
// (DevBuf, Events, the cloud staging) and fdm_engine_dem.inl (buildDEM), which it uses.  The header and ASCII records
// are host work (fdm_pcd_host.hpp); binary records are decoded and packed on the device (fdm_pcd.hpp).  Offline calls:
// synchronous, scratch is allocated per call.

#include "fdm_pcd_host.hpp"

namespace {
// fdm_pcd_debug_profile: the calling thread's decode / pack launches are timed with events, fdm_pcd_debug_last_kernel_ms
thread_local bool g_pcd_profile = false;
thread_local float g_pcd_ms[2] = {0.0f, 0.0f};

int pcd_kind(const fdm_pcd_field& f) {  // the branches of readFieldAsFloat (:209-230); anything else reads as 0
  if (f.type == 'F' && f.size == 4) return PCD_F4;
  if (f.type == 'F' && f.size == 8) return PCD_F8;
  if (f.type == 'U' && f.size == 1) return PCD_U1;
  if (f.type == 'U' && f.size == 4) return PCD_U4;
  if (f.type == 'I' && f.size == 4) return PCD_I4;
  return PCD_ZERO;
}
unsigned pcd_kind_bytes(int kind) { return kind == PCD_F8 ? 8u : (kind == PCD_U1 ? 1u : (kind == PCD_ZERO ? 0u : 4u)); }

// the eight channel indices of a header the caller filled (or fdm_pcd_parse_header did), checked
int pcd_indices(const fdm_pcd_header* h, int idx[8]) {
  if (!h) return fail(FDM_ERR_INVALID, "null header");
  if (h->n_fields < 0 || h->n_fields > FDM_PCD_MAX_FIELDS) return fail(FDM_ERR_INVALID, "PCD header: bad field count");
  const int32_t src[8] = {h->idx_x, h->idx_y, h->idx_z, h->idx_intensity, h->idx_rgb, h->idx_nx, h->idx_ny, h->idx_nz};
  for (int k = 0; k < 8; ++k) {
    if (src[k] >= h->n_fields) return fail(FDM_ERR_INVALID, "PCD header: a channel index is not a field");
    idx[k] = src[k] < 0 ? -1 : src[k];
  }
  if (idx[5] < 0 || idx[6] < 0 || idx[7] < 0) idx[5] = idx[6] = idx[7] = -1;  // the normal channel: all three or none (:289)
  return FDM_OK;
}

// What a binary decode of `h` reads: offsets and kinds of the present channels.  FDM_ERR_INVALID for the layouts the
// reference leaves undefined and for records beyond kPcdMaxPoint.
int pcd_plan(const fdm_pcd_header& h, const int idx[8], PcdDecode* D, bool* fields_aligned) {
  if (h.point_size == 0) return fail(FDM_ERR_INVALID, "PCD binary data with a point size of 0 (undefined in the reference)");
  if (h.point_size > kPcdMaxPoint) return fail(FDM_ERR_INVALID, "PCD binary records of more than 1024 bytes are not supported");
  *fields_aligned = (h.point_size & 3u) == 0;
  D->point_size = h.point_size;
  for (int k = 0; k < 8; ++k) {
    D->off[k] = 0;
    D->kind[k] = PCD_ZERO;
    if (idx[k] < 0) continue;
    const fdm_pcd_field& f = h.fields[idx[k]];
    const int kind = k == 4 ? PCD_U4 : pcd_kind(f);
    const unsigned width = pcd_kind_bytes(kind);
    if (uint64_t(f.offset) + width > h.point_size)
      return fail(FDM_ERR_INVALID, k == 4 ? "PCD colour field does not leave 4 bytes in the record (undefined in the reference)"
                                          : "PCD field reaches beyond the record (undefined in the reference)");
    D->off[k] = kind == PCD_ZERO ? 0 : int(f.offset);
    D->kind[k] = kind;
    if (width >= 4 && (f.offset & 3u)) *fields_aligned = false;
  }
  return FDM_OK;
}

// Binary records at d_body (device-visible) -> the device arrays D.out[]; synchronous on the null stream.
int pcd_decode_launch(const uint8_t* d_body, PcdDecode D, bool fields_aligned, uint64_t n) {
  const uintptr_t base = reinterpret_cast<uintptr_t>(d_body);
  if (D.point_size <= kPcdLdsMaxPoint) {
    D.stage = (base & 15u) == 0 ? 16 : ((base & 3u) == 0 ? 4 : 1);
    D.aligned = fields_aligned ? 1 : 0;  // (the slab starts on an LDS word whatever the base is)
  } else {
    D.stage = 0;
    D.aligned = fields_aligned && (base & 3u) == 0 ? 1 : 0;
  }
  const unsigned blocks = unsigned((n + kPcdBlockPoints - 1) / kPcdBlockPoints);
  Events E;
  if (g_pcd_profile) {
    if (int rc = E.init(2)) return rc;
    HIPCK(hipEventRecord(E.ev[0], nullptr));
  }
  hipLaunchKernelGGL(k_pcd_decode, dim3(blocks), dim3(256), 0, nullptr, d_body, D, (unsigned long long)n);
  HIPCK(hipGetLastError());
  if (g_pcd_profile) HIPCK(hipEventRecord(E.ev[1], nullptr));
  HIPCK(hipStreamSynchronize(nullptr));
  if (g_pcd_profile) g_pcd_ms[0] = E.ms(0, 1);
  return FDM_OK;
}

// loadPCD's data section into out[8] (x, y, z, intensity, rgb, nx, ny, nz; null = not wanted; a channel the file lacks is
// left alone): host or device arrays of width * height entries.
int pcd_decode_impl(const fdm_pcd_header* h, const void* body, uint64_t body_bytes, int body_on_device, void* const out[8],
                    int out_on_device, int device) {
  int idx[8];
  if (int rc = pcd_indices(h, idx)) return rc;
  const uint32_t n = h->width * h->height;  // PCDHeader::numPoints (:88)
  if (n == 0) return FDM_OK;                // :255
  if (idx[0] < 0 || idx[1] < 0 || idx[2] < 0) return fail(FDM_ERR_INVALID, "PCD file missing x, y, z fields");
  if (!body && body_bytes) return fail(FDM_ERR_INVALID, "null body");
  void* want[8];
  for (int k = 0; k < 8; ++k) want[k] = idx[k] >= 0 ? out[k] : nullptr;
  if (h->format == FDM_PCD_ASCII) {
    std::vector<char> host_body;
    const void* text = body;
    if (body_on_device && body_bytes) {
      if (int rc = pick_device(device)) return rc;
      host_body.resize(size_t(body_bytes));
      HIPCK(hipMemcpy(host_body.data(), body, size_t(body_bytes), hipMemcpyDeviceToHost));
      text = host_body.data();
    }
    std::vector<uint32_t> stage[8];
    void* dst[8];
    for (int k = 0; k < 8; ++k) {
      dst[k] = want[k];
      if (want[k] && out_on_device) {
        stage[k].resize(n);
        dst[k] = stage[k].data();
      }
    }
    fdm_pcd_header hh = *h;
    hh.idx_nx = idx[5]; hh.idx_ny = idx[6]; hh.idx_nz = idx[7];
    std::string error;
    if (fdm_pcd::parse_ascii(hh, text, size_t(body_bytes), static_cast<float*>(dst[0]), static_cast<float*>(dst[1]),
                             static_cast<float*>(dst[2]), static_cast<float*>(dst[3]), static_cast<uint32_t*>(dst[4]),
                             static_cast<float*>(dst[5]), static_cast<float*>(dst[6]), static_cast<float*>(dst[7]), &error))
      return fail(FDM_ERR_INVALID, error);
    if (out_on_device) {
      if (int rc = pick_device(device)) return rc;
      for (int k = 0; k < 8; ++k)
        if (want[k]) HIPCK(hipMemcpy(want[k], stage[k].data(), size_t(n) * 4, hipMemcpyHostToDevice));
    }
    return FDM_OK;
  }
  if (h->format != FDM_PCD_BINARY) return fail(FDM_ERR_INVALID, "PCD header: format is neither ascii nor binary");
  PcdDecode D{};
  bool fields_aligned = false;
  if (int rc = pcd_plan(*h, idx, &D, &fields_aligned)) return rc;
  const uint64_t need = uint64_t(n) * h->point_size;
  if (body_bytes < need) return fail(FDM_ERR_INVALID, "Unexpected end of binary data");
  if (int rc = pick_device(device)) return rc;
  DevBuf b_body;
  CloudBlock b_out;
  const uint8_t* d_body = static_cast<const uint8_t*>(body);
  if (!body_on_device) {
    const void* alias = pinned_alias(body);
    if (alias && (reinterpret_cast<uintptr_t>(alias) & 15u) == 0) {
      d_body = static_cast<const uint8_t*>(alias);  // pinned and on a 16-byte boundary: read in place, with the wide loads
    } else {  // pageable, or pinned at an odd offset (a copy from pinned memory costs less than byte-sized reads over PCIe)
      if (int rc = b_body.alloc(size_t(need))) return rc;
      HIPCK(hipMemcpy(b_body.p, body, size_t(need), hipMemcpyHostToDevice));
      d_body = b_body.as<uint8_t>();
    }
  }
  if (!out_on_device)
    if (int rc = b_out.alloc(n, 8)) return rc;
  for (int k = 0; k < 8; ++k) D.out[k] = !want[k] ? nullptr : (out_on_device ? want[k] : b_out.ch(k));
  if (int rc = pcd_decode_launch(d_body, D, fields_aligned, n)) return rc;
  if (!out_on_device)
    for (int k = 0; k < 8; ++k)
      if (want[k]) HIPCK(hipMemcpy(want[k], D.out[k], size_t(n) * 4, hipMemcpyDeviceToHost));
  return FDM_OK;
}

// savePCD's binary records of n device points: packed into d_rec (n * n_words words), downloaded into the host buffer
// `out`; synchronous on s
int pcd_pack_download(hipStream_t s, uint64_t n, const PcdPack& P, uint32_t* d_rec, void* out) {
  const size_t bytes = size_t(n) * size_t(P.n_words) * 4;
  Events E;
  if (g_pcd_profile) {
    if (int rc = E.init(2)) return rc;
    HIPCK(hipEventRecord(E.ev[0], s));
  }
  hipLaunchKernelGGL(k_pcd_pack, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, P, (unsigned long long)n, d_rec);
  HIPCK(hipGetLastError());
  if (g_pcd_profile) HIPCK(hipEventRecord(E.ev[1], s));
  HIPCK(hipMemcpyAsync(out, d_rec, bytes, hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (g_pcd_profile) g_pcd_ms[1] = E.ms(0, 1);
  return FDM_OK;
}
}  // namespace

extern "C" {

int fdm_pcd_debug_profile(int on) {
  g_pcd_profile = on != 0;
  g_pcd_ms[0] = g_pcd_ms[1] = 0.0f;
  return FDM_OK;
}

int fdm_pcd_debug_last_kernel_ms(float ms2[2]) {
  if (!ms2) return fail(FDM_ERR_INVALID, "null argument");
  ms2[0] = g_pcd_ms[0];
  ms2[1] = g_pcd_ms[1];
  return FDM_OK;
}

int fdm_pcd_parse_header(const void* bytes, uint64_t n_bytes, fdm_pcd_header* header) {
  if (!header || (!bytes && n_bytes)) return fail(FDM_ERR_INVALID, "null argument");
  std::string error;
  if (fdm_pcd::parse_header(bytes, size_t(n_bytes), header, &error)) return fail(FDM_ERR_INVALID, error);
  return FDM_OK;
}

int fdm_pcd_write_header(uint64_t n, int has_intensity, int has_rgb, int has_normal, const double* viewpoint, int format,
                         char* buf, uint64_t cap, uint64_t* n_bytes) {
  if (!n_bytes) return fail(FDM_ERR_INVALID, "null argument");
  *n_bytes = 0;
  if (format != FDM_PCD_ASCII && format != FDM_PCD_BINARY) return fail(FDM_ERR_INVALID, "format must be 0 (ascii) or 1 (binary)");
  const std::string text = fdm_pcd::write_header(n, has_intensity != 0, has_rgb != 0, has_normal != 0, viewpoint, format);
  *n_bytes = text.size();
  if (!buf || text.size() > cap) return FDM_SKIP_BUFFER_TOO_SMALL;
  std::memcpy(buf, text.data(), text.size());
  return FDM_OK;
}

int fdm_pcd_decode(const fdm_pcd_header* header, const void* body, uint64_t body_bytes, int body_on_device, float* x,
                   float* y, float* z, float* intensity, uint32_t* rgb, float* nx, float* ny, float* nz, int out_on_device,
                   int device) {
  void* const out[8] = {x, y, z, intensity, rgb, nx, ny, nz};
  return pcd_decode_impl(header, body, body_bytes, body_on_device, out, out_on_device, device);
}

int fdm_pcd_encode(uint64_t n, const float* x, const float* y, const float* z, const float* intensity, const uint32_t* rgb,
                   const float* nx, const float* ny, const float* nz, int on_device, int format, int precision, int device,
                   void* out, uint64_t cap, uint64_t* n_bytes) {
  if (!n_bytes) return fail(FDM_ERR_INVALID, "null argument");
  *n_bytes = 0;
  if (format != FDM_PCD_ASCII && format != FDM_PCD_BINARY) return fail(FDM_ERR_INVALID, "format must be 0 (ascii) or 1 (binary)");
  if (int rc = check_cloud(n, x, y, z)) return rc;
  const bool has_normal = nx && ny && nz;
  if (!has_normal && (nx || ny || nz)) return fail(FDM_ERR_INVALID, "the normal channel takes all three arrays or none");
  const void* ch[8] = {x, y, z, intensity, rgb, has_normal ? nx : nullptr, has_normal ? ny : nullptr, has_normal ? nz : nullptr};
  int n_words = 0;
  for (int k = 0; k < 8; ++k) n_words += ch[k] || k < 3 ? 1 : 0;
  if (n == 0) return FDM_OK;
  if (format == FDM_PCD_BINARY) {
    *n_bytes = n * uint64_t(n_words) * 4;
    if (!out || *n_bytes > cap) return FDM_SKIP_BUFFER_TOO_SMALL;
    if (int rc = pick_device(device)) return rc;
    CloudBlock b_in;
    PcdPack P{};
    P.n_words = n_words;
    if (int rc = stage_cloud(nullptr, n, 8, ch, on_device != 0, b_in, P.ch)) return rc;
    DevBuf b_rec;
    if (int rc = b_rec.alloc(size_t(*n_bytes))) return rc;
    return pcd_pack_download(nullptr, n, P, b_rec.as<uint32_t>(), out);
  }
  std::vector<uint32_t> host[8];
  if (on_device) {
    if (int rc = pick_device(device)) return rc;
    for (int k = 0; k < 8; ++k) {
      if (!ch[k]) continue;
      host[k].resize(size_t(n));
      HIPCK(hipMemcpy(host[k].data(), ch[k], size_t(n) * 4, hipMemcpyDeviceToHost));
      ch[k] = host[k].data();
    }
  }
  std::string text;
  fdm_pcd::format_ascii(n, static_cast<const float*>(ch[0]), static_cast<const float*>(ch[1]), static_cast<const float*>(ch[2]),
                        static_cast<const float*>(ch[3]), static_cast<const uint32_t*>(ch[4]), static_cast<const float*>(ch[5]),
                        static_cast<const float*>(ch[6]), static_cast<const float*>(ch[7]), precision, &text);
  *n_bytes = text.size();
  if (!out || text.size() > cap) return FDM_SKIP_BUFFER_TOO_SMALL;
  std::memcpy(out, text.data(), text.size());
  return FDM_OK;
}

// buildDEM(loadPCD(file), cfg): pcd2dem.cpp:38-44
int fdm_pcd_build_dem(const fdm_pcd_header* header, const void* body, uint64_t body_bytes, int body_on_device,
                      const fdm_dem_config* cfg, int device, fdm_engine** out_engine, fdm_dem_stats* stats) {
  if (stats) *stats = fdm_dem_stats{};
  if (!out_engine) return fail(FDM_ERR_INVALID, "null argument");
  *out_engine = nullptr;
  int idx[8];
  if (int rc = pcd_indices(header, idx)) return rc;
  const uint32_t n = header->width * header->height;
  if (n == 0) return fdm_engine_build_dem(0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, cfg, device, out_engine, stats);
  if (int rc = pick_device(device)) return rc;
  CloudBlock b_cloud;
  int slot[5], n_ch = 0;  // x, y, z and those of intensity, rgb the file has (buildDEM has no use for the normals)
  for (int k = 0; k < 5; ++k) slot[k] = k < 3 || idx[k] >= 0 ? n_ch++ : -1;
  if (int rc = b_cloud.alloc(n, n_ch)) return rc;
  void* out[8] = {};
  for (int k = 0; k < 5; ++k)
    if (slot[k] >= 0) out[k] = b_cloud.ch(slot[k]);
  if (int rc = pcd_decode_impl(header, body, body_bytes, body_on_device, out, 1, device)) return rc;
  return fdm_engine_build_dem(n, out[0], out[1], out[2], idx[3] >= 0 ? out[3] : nullptr, idx[4] >= 0 ? out[4] : nullptr, 1,
                              cfg, device, out_engine, stats);
}

// the binary data section of savePCD(toPointCloud(map)): pcd2dem.cpp:51-54
int fdm_engine_to_pcd(fdm_engine* e, void* out, uint64_t cap, uint64_t* n_bytes, uint64_t* n_points, int32_t* has_intensity,
                      int32_t* has_color) {
  if (!n_bytes || !n_points) return fail(FDM_ERR_INVALID, "null argument");
  *n_bytes = 0;
  const float *dx = nullptr, *dy = nullptr, *dz = nullptr, *di = nullptr;
  const uint32_t* dc = nullptr;
  int32_t hi = 0, hc = 0;
  if (int rc = fdm_engine_to_point_cloud_device(e, &dx, &dy, &dz, &di, &dc, n_points, &hi, &hc)) return rc;
  if (has_intensity) *has_intensity = hi;
  if (has_color) *has_color = hc;
  PcdPack P{};
  P.n_words = 3 + (hi ? 1 : 0) + (hc ? 1 : 0);
  P.ch[0] = dx; P.ch[1] = dy; P.ch[2] = dz;
  P.ch[3] = hi ? di : nullptr;
  P.ch[4] = hc ? dc : nullptr;
  *n_bytes = *n_points * uint64_t(P.n_words) * 4;
  if (*n_points == 0) return FDM_OK;
  if (!out || *n_bytes > cap) return FDM_SKIP_BUFFER_TOO_SMALL;
  const size_t words = size_t(*n_points) * size_t(P.n_words);
  // the engine's own record buffer: no allocation per call
  if (int rc = grow_device(e, &e->pcd_rec, &e->pcd_rec_cap, words, words + words / 4 + 1024)) return rc;
  return pcd_pack_download(e->stream, *n_points, P, e->pcd_rec, out);
}

}  // extern "C"
