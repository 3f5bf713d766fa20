// pcd_host_probe.cpp — the host half of the PCD codec (csrc/fdm_pcd_host.hpp) as a stand-alone program, so that it can
// run under AddressSanitizer / UndefinedBehaviorSanitizer without a device (tests/test_pcd_host_sanitized.py builds and
// runs it).  Every input is copied into a heap block of exactly its size first: a read behind the end is a report.
//
//   pcd_host_probe (header|sweep|ascii) FILE ...
//     header FILE   one line: the parse of FILE ("error", or "ok" and every value of the header)
//     sweep FILE    that line for every prefix of FILE, shortest first
//     ascii FILE    FILE's ASCII records parsed and written again at precision 8 and 3 ("error" where either parse fails)
#include "../../csrc/fdm_pcd_host.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <memory>

namespace {
std::string digest(const char* data, size_t n, fdm_pcd_header* h) {
  std::unique_ptr<char[]> exact(new char[n ? n : 1]);
  std::memcpy(exact.get(), data, n);
  std::string error;
  if (fdm_pcd::parse_header(exact.get(), n, h, &error)) return "error";
  char buf[256];
  std::snprintf(buf, sizeof(buf), "ok %d %u %u %u %d %llu %d %d %d %d %d %d %d %d", h->n_fields, h->width, h->height,
                h->point_size, h->format, static_cast<unsigned long long>(h->data_offset), h->idx_x, h->idx_y, h->idx_z,
                h->idx_intensity, h->idx_rgb, h->idx_nx, h->idx_ny, h->idx_nz);
  std::string out = buf;
  for (int i = 0; i < h->n_fields; ++i) {
    const fdm_pcd_field& f = h->fields[i];
    std::snprintf(buf, sizeof(buf), ":%d:%u:%u:%u", int(static_cast<unsigned char>(f.type)), f.size, f.count, f.offset);
    out += std::string(" ") + f.name + buf;
  }
  out += " vp";
  for (double v : h->viewpoint) {
    std::snprintf(buf, sizeof(buf), " %.17g", v);
    out += buf;
  }
  return out;
}

void ascii(const std::string& data) {
  fdm_pcd_header h;
  if (digest(data.data(), data.size(), &h) == "error") {
    std::printf("error\n");
    return;
  }
  const size_t n = size_t(h.width) * h.height, body_bytes = data.size() - size_t(h.data_offset);
  if (n > (1u << 20)) {
    std::printf("error\n");
    return;
  }
  std::unique_ptr<char[]> body(new char[body_bytes ? body_bytes : 1]);
  std::memcpy(body.get(), data.data() + h.data_offset, body_bytes);
  std::vector<float> ch[7];
  for (auto& v : ch) v.assign(n, 0.0f);
  std::vector<uint32_t> rgb(n, 0u);
  std::string error;
  if (fdm_pcd::parse_ascii(h, body.get(), body_bytes, ch[0].data(), ch[1].data(), ch[2].data(), ch[3].data(), rgb.data(),
                           ch[4].data(), ch[5].data(), ch[6].data(), &error)) {
    std::printf("error\n");
    return;
  }
  const bool has_normal = h.idx_nx >= 0 && h.idx_ny >= 0 && h.idx_nz >= 0;
  for (int precision : {8, 3}) {
    std::string text;
    fdm_pcd::format_ascii(n, ch[0].data(), ch[1].data(), ch[2].data(), h.idx_intensity >= 0 ? ch[3].data() : nullptr,
                          h.idx_rgb >= 0 ? rgb.data() : nullptr, has_normal ? ch[4].data() : nullptr,
                          has_normal ? ch[5].data() : nullptr, has_normal ? ch[6].data() : nullptr, precision, &text);
    std::printf("precision %d\n%s", precision, text.c_str());
  }
}
}  // namespace

int main(int argc, char** argv) {
  for (int a = 1; a + 1 < argc; a += 2) {
    const std::string mode = argv[a];
    std::ifstream f(argv[a + 1], std::ios::binary);
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[a + 1]);
      return 2;
    }
    const std::string data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::printf("== %s %s\n", mode.c_str(), argv[a + 1]);
    fdm_pcd_header h;
    if (mode == "header") {
      std::printf("%s\n", digest(data.data(), data.size(), &h).c_str());
    } else if (mode == "sweep") {
      for (size_t len = 0; len <= data.size(); ++len) std::printf("%s\n", digest(data.data(), len, &h).c_str());
    } else if (mode == "ascii") {
      ascii(data);
    } else {
      std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
      return 2;
    }
  }
  return 0;
}
