// voxel_order_npz — a LOCAL raycasting map built through the C++ host mirror (fastdem::FastDEM) with
// setVoxelAnyOrder(), written to an .npz for tests/test_voxel_order_mirror_gpu.py to hold against the oracle.
//
//   fdm_voxel_order_npz <dir> <stable|stdsort>
//
// <dir>/scans.bin: uint32 count, uint32 fork_at, double T_base_sensor[16] (row-major), then per scan uint32 n,
// float x[n], y[n], z[n], intensity[n], double T_world_base[16] (row-major).  Right before scan `fork_at` the map is
// replaced by a copy of itself (copy assignment: a new engine), so the mapper has to configure that engine again.
// Writes <dir>/out.npz: every layer (rows x cols, float32) and "_geometry" (int64: rows, cols, start_row, start_col).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "fastdem/fastdem.hpp"

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
  uint32_t u32() { return take<uint32_t>(1)[0]; }
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

// ---- .npz: an uncompressed zip of .npy members ----
uint32_t crc32(const std::string& s) {
  uint32_t c = 0xFFFFFFFFu;
  for (unsigned char ch : s) {
    c ^= ch;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}
std::string npy(const char* descr, bool fortran, const std::string& shape, const void* data, size_t bytes) {
  std::string h = std::string("{'descr': '") + descr + "', 'fortran_order': " + (fortran ? "True" : "False") +
                  ", 'shape': " + shape + ", }";
  while ((10 + h.size() + 1) % 64 != 0) h += ' ';
  h += '\n';
  std::string out("\x93NUMPY\x01\x00", 8);
  out += char(h.size() & 0xFF);
  out += char(h.size() >> 8);
  out += h;
  out.append(static_cast<const char*>(data), bytes);
  return out;
}
class Npz {
 public:
  void add(const std::string& name, const std::string& member) { m_.push_back({name + ".npy", member}); }
  void write(const std::string& file) const {
    std::string z, cd;
    auto u16 = [](std::string& s, uint32_t v) { s += char(v & 0xFF); s += char((v >> 8) & 0xFF); };
    auto u32 = [&](std::string& s, uint32_t v) { u16(s, v & 0xFFFF); u16(s, v >> 16); };
    for (const auto& e : m_) {
      const uint32_t crc = crc32(e.second), size = uint32_t(e.second.size()), at = uint32_t(z.size());
      u32(z, 0x04034b50u); u16(z, 20); u16(z, 0); u16(z, 0); u16(z, 0); u16(z, 0x21);
      u32(z, crc); u32(z, size); u32(z, size); u16(z, uint32_t(e.first.size())); u16(z, 0);
      z += e.first;
      z += e.second;
      u32(cd, 0x02014b50u); u16(cd, 20); u16(cd, 20); u16(cd, 0); u16(cd, 0); u16(cd, 0); u16(cd, 0x21);
      u32(cd, crc); u32(cd, size); u32(cd, size); u16(cd, uint32_t(e.first.size())); u16(cd, 0); u16(cd, 0);
      u16(cd, 0); u16(cd, 0); u32(cd, 0); u32(cd, at);
      cd += e.first;
    }
    const uint32_t cd_at = uint32_t(z.size());
    z += cd;
    u32(z, 0x06054b50u); u16(z, 0); u16(z, 0); u16(z, uint32_t(m_.size())); u16(z, uint32_t(m_.size()));
    u32(z, uint32_t(cd.size())); u32(z, cd_at); u16(z, 0);
    std::FILE* f = std::fopen(file.c_str(), "wb");
    if (!f || std::fwrite(z.data(), 1, z.size(), f) != z.size()) throw std::runtime_error("cannot write " + file);
    std::fclose(f);
  }

 private:
  std::vector<std::pair<std::string, std::string>> m_;
};

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc != 3) throw std::runtime_error("usage: fdm_voxel_order_npz <dir> <stable|stdsort>");
    const std::string dir = argv[1], order = argv[2];
    Reader in(dir + "/scans.bin");
    const uint32_t count = in.u32(), fork_at = in.u32();
    const Eigen::Isometry3d Tbs = in.pose();

    ElevationMap map(24.0f, 24.0f, 0.1f, "map");
    FastDEM mapper(map);
    mapper.setMappingMode(MappingMode::LOCAL).setHeightFilter(-2.0f, 4.0f).setRangeFilter(0.2f, 14.0f);
    mapper.enableRaycasting(true);
    mapper.setVoxelAnyOrder(order == "stdsort" ? VoxelAnyOrder::StdSort : VoxelAnyOrder::Stable);
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t n = in.u32();
      const std::vector<float> x = in.take<float>(n), y = in.take<float>(n), z = in.take<float>(n),
                               it = in.take<float>(n);
      const Eigen::Isometry3d Twb = in.pose();
      if (k == fork_at) {
        const ElevationMap copy(map);
        map = copy;  // another engine under the same map: the mapper configures it before the next scan
      }
      PointCloud c;
      c.resize(n);
      c.useIntensity();
      for (uint32_t i = 0; i < n; ++i) {
        c.point(i) = Eigen::Vector3f(x[i], y[i], z[i]);
        c.intensity(i) = it[i];
      }
      mapper.integrate(c, Tbs, Twb);
    }
    Npz out;
    const nanogrid::Size sz = map.getSize();
    const nanogrid::Index st = map.getStartIndex();
    const std::string shape = "(" + std::to_string(sz(0)) + ", " + std::to_string(sz(1)) + ")";
    for (const auto& name : map.getLayers()) {  // column-major as the mirror holds it
      const nanogrid::Matrix& a = map.get(name);
      out.add(name, npy("<f4", true, shape, a.data(), size_t(a.size()) * sizeof(float)));
    }
    const int64_t g[4] = {sz(0), sz(1), st(0), st(1)};
    out.add("_geometry", npy("<i8", false, "(4,)", g, sizeof(g)));
    out.write(dir + "/out.npz");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fdm_voxel_order_npz: %s\n", e.what());
    return 1;
  }
}
