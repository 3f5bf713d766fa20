// fastdem/io/crc32.hpp — the CRC-32 both file writers of this directory need (ZIP members of io/npz.hpp, PNG chunks of
// io/png.hpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace fastdem {
namespace io {
namespace detail {

inline uint32_t crc32(const void* data, size_t len) {  // IEEE 802.3, reflected, poly 0xEDB88320
  static uint32_t table[256];
  static bool ready = false;
  if (!ready) {
    for (uint32_t n = 0; n < 256; ++n) {
      uint32_t c = n;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
      table[n] = c;
    }
    ready = true;
  }
  uint32_t crc = ~0u;
  const uint8_t* p = static_cast<const uint8_t*>(data);
  for (size_t i = 0; i < len; ++i) crc = table[(crc ^ p[i]) & 0xFFu] ^ (crc >> 8);
  return ~crc;
}

}  // namespace detail
}  // namespace io
}  // namespace fastdem
