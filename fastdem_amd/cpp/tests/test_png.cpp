// test_png — fastdem::io::savePng through the C++ host mirror (tests/test_png_file.py decodes the files and holds
// them against the engine's pixels for the same scans).
//
//   fdm_test_png <dir>
//
// <dir>/scans.bin: uint32 count, double T_base_sensor[16] (row-major), then per scan uint32 n, float x[n], y[n], z[n],
// double T_world_base[16] (row-major); then double move_x, move_y.  A 64 x 48-cell LOCAL map integrates the scans, is
// moved to (move_x, move_y) and written as <dir>/default.png (elevation, PngExportConfig{}), <dir>/minmax_jet.png
// (variance, MIN_MAX + JET, not aligned) and <dir>/fixed_gray.png (elevation, FIXED_RANGE -0.2 .. 0.25 + GRAYSCALE).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "fastdem/fastdem.hpp"
#include "fastdem/io/png.hpp"

using namespace fastdem;

namespace {
class Reader {
 public:
  explicit Reader(const std::string& file) {
    std::ifstream f(file, std::ios::binary);
    if (!f) throw std::runtime_error("cannot read " + file);
    b_.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  }
  template <typename T>
  std::vector<T> take(size_t n) {
    if (off_ + n * sizeof(T) > b_.size()) throw std::runtime_error("scans.bin is truncated");
    std::vector<T> v(n);
    std::memcpy(v.data(), b_.data() + off_, n * sizeof(T));
    off_ += n * sizeof(T);
    return v;
  }
  Eigen::Isometry3d pose() {
    const std::vector<double> m = take<double>(16);
    Eigen::Isometry3d T = Eigen::Isometry3d::Identity();
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) T.data()[c * 4 + r] = m[size_t(r) * 4 + size_t(c)];
    return T;
  }

 private:
  std::vector<char> b_;
  size_t off_ = 0;
};

bool exists(const std::string& file) { return std::ifstream(file, std::ios::binary).good(); }
void expect(bool ok, const char* what) {
  if (!ok) throw std::runtime_error(std::string("expectation failed: ") + what);
}
}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc != 2) throw std::runtime_error("usage: fdm_test_png <dir>");
    const std::string dir = argv[1];
    Reader in(dir + "/scans.bin");
    const uint32_t count = in.take<uint32_t>(1)[0];
    const Eigen::Isometry3d Tbs = in.pose();

    ElevationMap map(6.4f, 4.8f, 0.1f, "map");
    FastDEM mapper(map);
    mapper.setMappingMode(MappingMode::LOCAL);
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t n = in.take<uint32_t>(1)[0];
      const std::vector<float> x = in.take<float>(n), y = in.take<float>(n), z = in.take<float>(n);
      const Eigen::Isometry3d Twb = in.pose();
      PointCloud c;
      c.resize(n);
      for (uint32_t i = 0; i < n; ++i) c.point(i) = Eigen::Vector3f(x[i], y[i], z[i]);
      expect(mapper.integrate(c, Tbs, Twb), "integrate");
    }
    const std::vector<double> to = in.take<double>(2);
    map.move(nanogrid::Position(to[0], to[1]));
    const nanogrid::Index st = map.getStartIndex();
    expect(st(0) != 0 && st(1) != 0, "the start index is non-zero on both axes");

    expect(io::savePng(dir + "/default.png", map, layer::elevation), "savePng with the default config");
    io::PngExportConfig cfg;
    expect(cfg.normalize == io::PngExportConfig::Normalize::PERCENTILE_1_99 &&
               cfg.colormap == io::PngExportConfig::Colormap::VIRIDIS && cfg.align_to_world && cfg.fixed_min == -2.0f &&
               cfg.fixed_max == 2.0f, "PngExportConfig{} defaults");
    cfg.normalize = io::PngExportConfig::Normalize::MIN_MAX;
    cfg.colormap = io::PngExportConfig::Colormap::JET;
    cfg.align_to_world = false;
    expect(io::savePng(dir + "/minmax_jet.png", map, layer::variance, cfg), "savePng MIN_MAX + JET");
    cfg.normalize = io::PngExportConfig::Normalize::FIXED_RANGE;
    cfg.colormap = io::PngExportConfig::Colormap::GRAYSCALE;
    cfg.align_to_world = true;
    cfg.fixed_min = -0.2f;
    cfg.fixed_max = 0.25f;
    expect(io::savePng(dir + "/fixed_gray.png", map, layer::elevation, cfg), "savePng FIXED_RANGE + GRAYSCALE");

    // a missing layer: false, and no file; a file that cannot be created: false
    expect(!io::savePng(dir + "/missing.png", map, "no_such_layer"), "a missing layer returns false");
    expect(!exists(dir + "/missing.png"), "a missing layer creates no file");
    expect(!io::savePng(dir + "/no_such_dir/x.png", map, layer::elevation), "a write failure returns false");
    std::printf("start %d %d\npng: ok\n", st(0), st(1));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fdm_test_png: %s\n", e.what());
    return 1;
  }
}
