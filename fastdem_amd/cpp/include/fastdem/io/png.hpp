// fastdem/io/png.hpp — ElevationMap layer -> colour-mapped PNG
// (API: fastdem/include/fastdem/io/png.hpp:27-43; pixels: fastdem/src/io_png.cpp).
//
// The pixels are computed on the device (fdm_engine_render_layer: normalisation range by radix select, colour map,
// circular-buffer unrolling) and are exactly the reference's; the host receives one RGBA copy and writes the file.
//
// File format: 8-bit RGBA, non-interlaced, filter type 0 on every scanline, ONE IDAT chunk whose zlib stream is made
// of *stored* deflate blocks (no compression, no dependency).  The file is a valid PNG with the same pixels as the
// reference's, NOT the same bytes: the reference compresses through stb_image_write.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "fastdem/elevation_map.hpp"
#include "fastdem/io/crc32.hpp"

namespace fastdem {
namespace io {

/// Configuration for PNG image export.
struct PngExportConfig {
  enum class Normalize { MIN_MAX, PERCENTILE_1_99, FIXED_RANGE };
  enum class Colormap { GRAYSCALE, VIRIDIS, JET };

  Normalize normalize = Normalize::PERCENTILE_1_99;
  Colormap colormap = Colormap::VIRIDIS;
  bool align_to_world = true;  // unroll the circular buffer
  float fixed_min = -2.0f;     // for FIXED_RANGE
  float fixed_max = 2.0f;
};

namespace detail {

inline void pngBe32(std::string& b, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) b.push_back(char((v >> s) & 0xFFu));
}
inline void pngChunk(std::string& out, const char type[4], const std::string& data) {
  pngBe32(out, uint32_t(data.size()));
  const size_t at = out.size();
  out.append(type, 4);
  out.append(data);
  pngBe32(out, crc32(out.data() + at, out.size() - at));  // over type + data
}

// zlib stream (RFC 1950) of stored deflate blocks (RFC 1951 §3.2.4) of at most 65 535 bytes, Adler-32 at the end
inline std::string zlibStored(const uint8_t* raw, size_t len) {
  std::string z;
  z.reserve(len + 5 * (len / 65535 + 1) + 6);
  z.push_back(char(0x78));
  z.push_back(char(0x01));  // (0x7801 is a multiple of 31; no preset dictionary, fastest level)
  uint32_t a = 1, b = 0;    // Adler-32: sums modulo 65521, reduced before 32 bits can overflow
  size_t at = 0;
  do {
    const size_t n = len - at < 65535 ? len - at : 65535;
    z.push_back(char(at + n == len ? 1 : 0));  // BFINAL, BTYPE = 00
    z.push_back(char(n & 0xFF)); z.push_back(char(n >> 8));
    z.push_back(char(~n & 0xFF)); z.push_back(char((~n >> 8) & 0xFF));
    z.append(reinterpret_cast<const char*>(raw + at), n);
    for (size_t k = at; k < at + n;) {
      const size_t stop = at + n - k < 5552 ? at + n : k + 5552;
      for (; k < stop; ++k) { a += raw[k]; b += a; }
      a %= 65521u; b %= 65521u;
    }
    at += n;
  } while (at < len);
  pngBe32(z, (b << 16) | a);
  return z;
}

/// Row-major RGBA8 pixels -> PNG file.  false: empty image, or the file could not be written.
inline bool writePngRgba8(const std::string& filename, const uint8_t* rgba, uint32_t width, uint32_t height) {
  if (!rgba || width == 0 || height == 0) return false;
  const size_t line = size_t(width) * 4;
  std::vector<uint8_t> raw((line + 1) * height);
  for (uint32_t r = 0; r < height; ++r) {
    raw[(line + 1) * r] = 0;  // filter type 0 (None)
    std::copy(rgba + line * r, rgba + line * (r + 1), raw.begin() + std::ptrdiff_t((line + 1) * r + 1));
  }
  std::string file("\x89PNG\r\n\x1a\n", 8);
  std::string ihdr;
  pngBe32(ihdr, width);
  pngBe32(ihdr, height);
  ihdr.append("\x08\x06\x00\x00\x00", 5);  // bit depth 8, colour type 6 (RGBA), deflate, adaptive filtering, no interlace
  pngChunk(file, "IHDR", ihdr);
  pngChunk(file, "IDAT", zlibStored(raw.data(), raw.size()));
  pngChunk(file, "IEND", std::string());
  std::ofstream fs(filename, std::ios::binary);
  if (!fs.is_open()) return false;
  fs.write(file.data(), std::streamsize(file.size()));
  fs.close();
  return !fs.fail();
}

}  // namespace detail

/// Export ElevationMap layer as PNG image with colormap (io_png.cpp:115-171).
inline bool savePng(const std::string& filename, const ElevationMap& map, const std::string& layer_name,
                    const PngExportConfig& config = {}) {
  if (!map.exists(layer_name)) {
    std::fprintf(stderr, "[png_io] Layer '%s' does not exist\n", layer_name.c_str());
    return false;
  }
  const_cast<ElevationMap&>(map).flushToDevice();  // host-side writes of the layer are part of the picture
  fdm_image_config cfg;
  cfg.normalize = int32_t(config.normalize);
  cfg.colormap = int32_t(config.colormap);
  cfg.align_to_world = config.align_to_world ? 1 : 0;
  cfg.fixed_min = config.fixed_min;
  cfg.fixed_max = config.fixed_max;
  int32_t width = 0, height = 0;
  if (fdm_engine_render_layer(map.engine(), layer_name.c_str(), &cfg, nullptr, 0, &width, &height, nullptr) != FDM_OK ||
      width <= 0 || height <= 0) {
    std::fprintf(stderr, "[png_io] Render failed for layer '%s': %s\n", layer_name.c_str(), fdm_last_error());
    return false;
  }
  std::vector<uint8_t> pixels(size_t(width) * size_t(height) * 4);
  if (fdm_engine_render_layer(map.engine(), layer_name.c_str(), &cfg, pixels.data(), pixels.size(), &width, &height,
                              nullptr) != FDM_OK) {
    std::fprintf(stderr, "[png_io] Render failed for layer '%s': %s\n", layer_name.c_str(), fdm_last_error());
    return false;
  }
  if (!detail::writePngRgba8(filename, pixels.data(), uint32_t(width), uint32_t(height))) {
    std::fprintf(stderr, "[png_io] Write failed for %s\n", filename.c_str());
    return false;
  }
  return true;
}

}  // namespace io
}  // namespace fastdem
