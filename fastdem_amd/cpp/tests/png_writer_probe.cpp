// png_writer_probe — the header-only PNG writer of fastdem/io/png.hpp on fixed RGBA patterns, no device involved
// (tests/test_png_file.py decodes the files).
//
//   fdm_png_writer_probe <dir>
//
// Writes <dir>/big.png (150 x 130: 78 130 scanline bytes, more than one 65 535-byte stored block), <dir>/edge.png
// (4 x 3 855: exactly 65 535 scanline bytes) and <dir>/one.png (1 x 1).  Pixel (r, c), channel k holds
// (7 r + 13 c + 29 k + r c) mod 256.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "fastdem/io/png.hpp"

namespace {
bool write(const std::string& file, uint32_t width, uint32_t height) {
  std::vector<uint8_t> px(size_t(width) * height * 4);
  for (uint32_t r = 0; r < height; ++r)
    for (uint32_t c = 0; c < width; ++c)
      for (uint32_t k = 0; k < 4; ++k) px[(size_t(r) * width + c) * 4 + k] = uint8_t(7u * r + 13u * c + 29u * k + r * c);
  return fastdem::io::detail::writePngRgba8(file, px.data(), width, height);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: fdm_png_writer_probe <dir>\n");
    return 2;
  }
  const std::string dir = argv[1];
  // 3 855 scanlines of 1 + 4 * 4 = 17 bytes are exactly 65 535: the stream is one full stored block, nothing after it
  const bool ok = write(dir + "/big.png", 150, 130) && write(dir + "/edge.png", 4, 3855) && write(dir + "/one.png", 1, 1);
  // a file that cannot be created and an empty image are refused
  const bool refused = !write(dir + "/no_such_dir/x.png", 2, 2) &&
                       !fastdem::io::detail::writePngRgba8(dir + "/empty.png", nullptr, 0, 0);
  std::printf("written %d refused %d\n", int(ok), int(refused));
  return ok && refused ? 0 : 1;
}
