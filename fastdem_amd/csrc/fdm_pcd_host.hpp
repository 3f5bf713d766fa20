// fdm_pcd_host.hpp — the host half of the PCD codec: header parser and writer, ASCII record parser and formatter.
// Plain C++17, no HIP: it compiles into libfdm_engine.so (fdm_engine_pcd.inl) and into stand-alone programs
// (cpp/tests/pcd_host_probe.cpp runs it under the sanitizers).
//
// Reference being reproduced: fastdem/lib/nanoPCL/include/nanopcl/io/pcd_io.hpp — parseHeader :114-207, the ASCII
// branch of loadPCD :296-331, savePCD's header :454-488 and ASCII records :490-514.  Where the reference would index a
// missing token (:150, :152) or throw from std::stoul / std::stod / std::stof, this returns an error; no byte behind
// `n_bytes` is ever read.
#pragma once

#include "../../include/fdm_engine.h"

#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace fdm_pcd {

struct Token {
  const char* p;
  size_t len;
};

// what `iss >> token` skips: the "C" locale's isspace
inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// detail::split (:104-112) over [p, end)
inline void split(const char* p, const char* end, std::vector<Token>* out) {
  out->clear();
  while (p < end) {
    while (p < end && is_space(*p)) ++p;
    if (p >= end) break;
    const char* q = p;
    while (q < end && !is_space(*q)) ++q;
    out->push_back(Token{p, size_t(q - p)});
    p = q;
  }
}

// std::getline over [*pos, end): false at the end of the buffer with nothing left; the line excludes its '\n'
inline bool next_line(const char** pos, const char* end, const char** line, const char** line_end) {
  if (*pos >= end) return false;
  const char* nl = static_cast<const char*>(std::memchr(*pos, '\n', size_t(end - *pos)));
  *line = *pos;
  *line_end = nl ? nl : end;
  *pos = nl ? nl + 1 : end;
  return true;
}

inline std::string lower(const Token& t) {
  std::string s(t.p, t.len);
  for (char& c : s) c = char(std::tolower(static_cast<unsigned char>(c)));
  return s;
}

// std::stoul(token) narrowed to uint32_t as the reference's assignments narrow it: false where stoul throws
inline bool to_u32(const Token& t, uint32_t* out) {
  const std::string s(t.p, t.len);
  char* endp = nullptr;
  errno = 0;
  const unsigned long v = std::strtoul(s.c_str(), &endp, 10);
  if (endp == s.c_str() || errno == ERANGE) return false;
  *out = uint32_t(v);
  return true;
}
inline bool to_f64(const Token& t, double* out) {  // std::stod
  const std::string s(t.p, t.len);
  char* endp = nullptr;
  errno = 0;
  const double v = std::strtod(s.c_str(), &endp);
  if (endp == s.c_str() || errno == ERANGE) return false;
  *out = v;
  return true;
}
inline bool to_f32(const Token& t, float* out) {  // std::stof
  const std::string s(t.p, t.len);
  char* endp = nullptr;
  errno = 0;
  const float v = std::strtof(s.c_str(), &endp);
  if (endp == s.c_str() || errno == ERANGE) return false;
  *out = v;
  return true;
}

inline int find_field(const fdm_pcd_header& h, const char* name) {  // PCDHeader::findField (:90-95)
  for (int i = 0; i < h.n_fields; ++i)
    if (std::strcmp(h.fields[i].name, name) == 0) return i;
  return -1;
}

inline int err(std::string* e, const char* msg) {
  if (e) *e = msg;
  return -1;
}

// parseHeader (:114-207) and loadPCD's field choice (:260-281).  0, or -1 with *error set.
inline int parse_header(const void* bytes, size_t n_bytes, fdm_pcd_header* h, std::string* error) {
  std::memset(h, 0, sizeof(*h));
  h->height = 1;
  h->viewpoint[3] = 1.0;  // identity: t = 0, q = (1, 0, 0, 0)
  h->format = FDM_PCD_ASCII;
  const char* pos = static_cast<const char*>(bytes);
  const char* const end = pos + n_bytes;
  std::vector<std::string> names;
  uint32_t sizes[FDM_PCD_MAX_FIELDS], counts[FDM_PCD_MAX_FIELDS];
  char types[FDM_PCD_MAX_FIELDS];
  size_t n_sizes = 0, n_types = 0, n_counts = 0;  // entries behind FDM_PCD_MAX_FIELDS are counted, not kept
  std::vector<Token> tok;
  const char *line, *line_end;
  while (next_line(&pos, end, &line, &line_end)) {
    if (line == line_end || *line == '#') continue;
    split(line, line_end, &tok);
    if (tok.empty()) continue;
    const std::string key = lower(tok[0]);
    if (key == "fields") {
      for (size_t i = 1; i < tok.size(); ++i) {
        if (names.size() >= size_t(FDM_PCD_MAX_FIELDS)) return err(error, "PCD header has more than 64 fields");
        names.push_back(lower(tok[i]));
      }
    } else if (key == "size" || key == "count") {
      uint32_t* const dst = key == "size" ? sizes : counts;
      size_t& cnt = key == "size" ? n_sizes : n_counts;
      for (size_t i = 1; i < tok.size(); ++i) {
        uint32_t v;
        if (!to_u32(tok[i], &v)) return err(error, "PCD header: SIZE / COUNT entry is not a number");
        if (cnt < size_t(FDM_PCD_MAX_FIELDS)) dst[cnt] = v;
        ++cnt;
      }
    } else if (key == "type") {
      for (size_t i = 1; i < tok.size(); ++i) {
        if (n_types < size_t(FDM_PCD_MAX_FIELDS)) types[n_types] = tok[i].p[0];
        ++n_types;
      }
    } else if (key == "width" || key == "height") {
      if (tok.size() < 2) return err(error, "PCD header: WIDTH / HEIGHT without a number");
      if (!to_u32(tok[1], key == "width" ? &h->width : &h->height))
        return err(error, "PCD header: WIDTH / HEIGHT is not a number");
    } else if (key == "viewpoint") {
      if (tok.size() >= 8) {
        double v[7];
        for (int k = 0; k < 7; ++k)
          if (!to_f64(tok[size_t(k) + 1], &v[k])) return err(error, "PCD header: VIEWPOINT entry is not a number");
        for (int k = 0; k < 7; ++k) h->viewpoint[k] = v[k];
      }
    } else if (key == "data") {
      if (tok.size() >= 2) {
        const std::string fmt = lower(tok[1]);
        if (fmt == "ascii") h->format = FDM_PCD_ASCII;
        else if (fmt == "binary") h->format = FDM_PCD_BINARY;
        else if (fmt == "binary_compressed") return err(error, "PCD binary_compressed format not supported");
      }
      break;  // DATA is the last header line
    }  // version, points, anything else: ignored
  }
  h->data_offset = uint64_t(pos - static_cast<const char*>(bytes));
  if (names.empty()) return err(error, "PCD header missing FIELDS");
  uint32_t offset = 0;
  h->n_fields = int32_t(names.size());
  for (size_t i = 0; i < names.size(); ++i) {
    fdm_pcd_field& f = h->fields[i];
    std::snprintf(f.name, sizeof(f.name), "%s", names[i].c_str());  // (a name of 64 characters or more matches no channel)
    f.size = i < n_sizes ? sizes[i] : 4u;
    f.type = i < n_types ? types[i] : 'F';
    f.count = i < n_counts ? counts[i] : 1u;
    f.offset = offset;
    offset += f.size * f.count;  // uint32 arithmetic, as the reference's
  }
  h->point_size = offset;
  auto first_of = [&](std::initializer_list<const char*> alias) {
    for (const char* a : alias)
      if (int i = find_field(*h, a); i >= 0) return i;
    return -1;
  };
  h->idx_x = find_field(*h, "x");
  h->idx_y = find_field(*h, "y");
  h->idx_z = find_field(*h, "z");
  h->idx_intensity = first_of({"intensity", "i", "reflectivity"});
  h->idx_rgb = first_of({"rgb", "rgba"});
  h->idx_nx = first_of({"normal_x", "nx"});
  h->idx_ny = first_of({"normal_y", "ny"});
  h->idx_nz = first_of({"normal_z", "nz"});
  return 0;
}

// savePCD's header (:454-488, :491 / :516): exactly its text
inline std::string write_header(uint64_t n, bool has_intensity, bool has_rgb, bool has_normal, const double viewpoint[7],
                                int format) {
  std::string fields = "x y z", sizes = "4 4 4", types = "F F F", counts = "1 1 1";
  auto add = [&](const char* name, const char* type) {
    fields += std::string(" ") + name;
    sizes += " 4";
    types += std::string(" ") + type;
    counts += " 1";
  };
  if (has_intensity) add("intensity", "F");
  if (has_rgb) add("rgb", "U");
  if (has_normal) {
    add("normal_x", "F");
    add("normal_y", "F");
    add("normal_z", "F");
  }
  static const double kIdentity[7] = {0, 0, 0, 1, 0, 0, 0};
  const double* vp = viewpoint ? viewpoint : kIdentity;
  char num[64];
  std::string out = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\n";
  out += "FIELDS " + fields + "\nSIZE " + sizes + "\nTYPE " + types + "\nCOUNT " + counts + "\n";
  std::snprintf(num, sizeof(num), "%llu", static_cast<unsigned long long>(n));
  out += std::string("WIDTH ") + num + "\nHEIGHT 1\nVIEWPOINT";
  for (int k = 0; k < 7; ++k) {
    char g[64];
    std::snprintf(g, sizeof(g), " %g", vp[k]);  // operator<<(double) at the stream's defaults
    out += g;
  }
  out += std::string("\nPOINTS ") + num + "\n";
  out += format == FDM_PCD_ASCII ? "DATA ascii\n" : "DATA binary\n";
  return out;
}

// The ASCII branch of loadPCD (:296-331): one line per point, the value of a field is the token at the field's INDEX
// (COUNT is not accounted for, as in the reference).  Output arrays of width * height entries, any may be null.
inline int parse_ascii(const fdm_pcd_header& h, const void* body, size_t body_bytes, float* x, float* y, float* z,
                       float* intensity, uint32_t* rgb, float* nx, float* ny, float* nz, std::string* error) {
  const uint32_t n = h.width * h.height;
  if (n == 0) return 0;
  if (h.idx_x < 0 || h.idx_y < 0 || h.idx_z < 0) return err(error, "PCD file missing x, y, z fields");
  const bool has_normal = h.idx_nx >= 0 && h.idx_ny >= 0 && h.idx_nz >= 0;
  const char* pos = static_cast<const char*>(body);
  const char* const end = pos + body_bytes;
  std::vector<Token> tok;
  const char *line, *line_end;
  for (uint32_t i = 0; i < n; ++i) {
    if (!next_line(&pos, end, &line, &line_end)) return err(error, "Unexpected end of ASCII data");
    split(line, line_end, &tok);
    if (tok.size() < size_t(h.n_fields)) return err(error, "Incomplete point data");
    float v[3];
    if (!to_f32(tok[size_t(h.idx_x)], &v[0]) || !to_f32(tok[size_t(h.idx_y)], &v[1]) || !to_f32(tok[size_t(h.idx_z)], &v[2]))
      return err(error, "PCD ASCII data: a coordinate is not a number");
    if (x) x[i] = v[0];
    if (y) y[i] = v[1];
    if (z) z[i] = v[2];
    if (h.idx_intensity >= 0) {
      float a;
      if (!to_f32(tok[size_t(h.idx_intensity)], &a)) return err(error, "PCD ASCII data: an intensity is not a number");
      if (intensity) intensity[i] = a;
    }
    if (h.idx_rgb >= 0) {
      uint32_t c;
      if (!to_u32(tok[size_t(h.idx_rgb)], &c)) return err(error, "PCD ASCII data: a colour is not an integer");
      if (rgb) rgb[i] = c & 0x00FFFFFFu;
    }
    if (has_normal) {
      float m[3];
      if (!to_f32(tok[size_t(h.idx_nx)], &m[0]) || !to_f32(tok[size_t(h.idx_ny)], &m[1]) || !to_f32(tok[size_t(h.idx_nz)], &m[2]))
        return err(error, "PCD ASCII data: a normal is not a number");
      if (nx) nx[i] = m[0];
      if (ny) ny[i] = m[1];
      if (nz) nz[i] = m[2];
    }
  }
  return 0;
}

// savePCD's ASCII records (:492-514): std::fixed at `precision`, the colour as a decimal integer.  intensity, rgb and
// the normals (all three or none) may be null: the channel is absent.
inline void format_ascii(uint64_t n, const float* x, const float* y, const float* z, const float* intensity,
                         const uint32_t* rgb, const float* nx, const float* ny, const float* nz, int precision,
                         std::string* out) {
  if (precision < 0) precision = 6;  // what std::num_put makes of a negative precision
  std::vector<char> buf(size_t(precision) + 64);
  auto put = [&](float v) {
    const int len = std::snprintf(buf.data(), buf.size(), "%.*f", precision, double(v));
    out->append(buf.data(), size_t(len));
  };
  const bool has_normal = nx && ny && nz;
  for (uint64_t i = 0; i < n; ++i) {
    put(x[i]);
    out->push_back(' ');
    put(y[i]);
    out->push_back(' ');
    put(z[i]);
    if (intensity) {
      out->push_back(' ');
      put(intensity[i]);
    }
    if (rgb) {
      const int len = std::snprintf(buf.data(), buf.size(), " %u", unsigned(rgb[i] & 0x00FFFFFFu));
      out->append(buf.data(), size_t(len));
    }
    if (has_normal) {
      out->push_back(' ');
      put(nx[i]);
      out->push_back(' ');
      put(ny[i]);
      out->push_back(' ');
      put(nz[i]);
    }
    out->push_back('\n');
  }
}

}  // namespace fdm_pcd
