// nanopcl/io/pcd_io.hpp — the surface of the reference's nanopcl/io/pcd_io.hpp (PCDFormat, PCDMetadata, PCDSaveOptions,
// IOException, loadPCD / savePCD for streams and paths) over the C ABI: the header and ASCII records are parsed by
// fdm_pcd_parse_header / fdm_pcd_decode on the host, binary records are decoded and packed on the device
// (fdm_pcd_decode, fdm_pcd_encode).  A file read by path has its data section in a pinned block of its own, 16-byte
// aligned, which the device reads in place.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "nanopcl/core.hpp"

namespace nanopcl {
namespace io {

class IOException : public std::runtime_error {
 public:
  using std::runtime_error::runtime_error;
};

enum class PCDFormat { ASCII, BINARY };

/// Metadata from the PCD file header
struct PCDMetadata {
  Eigen::Isometry3d viewpoint = Eigen::Isometry3d::Identity();
  uint32_t width = 0;
  uint32_t height = 1;
  uint32_t num_points = 0;
};

/// Options for saving PCD files
struct PCDSaveOptions {
  PCDFormat format = PCDFormat::BINARY;
  Eigen::Isometry3d viewpoint = Eigen::Isometry3d::Identity();
  int precision = 8;  // for the ASCII format
};

namespace detail {

// Eigen::Quaterniond(w, x, y, z).toRotationMatrix(), by Eigen's documented formula (the quaternion is not normalised)
inline Eigen::Matrix3d quaternionToRotation(double w, double x, double y, double z) {
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  Eigen::Matrix3d R;
  R(0, 0) = 1.0 - (tyy + tzz); R(0, 1) = txy - twz;         R(0, 2) = txz + twy;
  R(1, 0) = txy + twz;         R(1, 1) = 1.0 - (txx + tzz); R(1, 2) = tyz - twx;
  R(2, 0) = txz - twy;         R(2, 1) = tyz + twx;         R(2, 2) = 1.0 - (txx + tyy);
  return R;
}

// Eigen::Quaterniond(R): q[0..3] = w, x, y, z, by the branch on the trace and the largest diagonal entry Eigen documents
inline void rotationToQuaternion(const Eigen::Matrix3d& m, double q[4]) {
  double t = m(0, 0) + m(1, 1) + m(2, 2);
  if (t > 0.0) {
    t = std::sqrt(t + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (m(2, 1) - m(1, 2)) * t;
    q[2] = (m(0, 2) - m(2, 0)) * t;
    q[3] = (m(1, 0) - m(0, 1)) * t;
  } else {
    int i = 0;
    if (m(1, 1) > m(0, 0)) i = 1;
    if (m(2, 2) > m(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0);
    q[1 + i] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m(k, j) - m(j, k)) * t;
    q[1 + j] = (m(j, i) + m(i, j)) * t;
    q[1 + k] = (m(k, i) + m(i, k)) * t;
  }
}

inline void viewpointNumbers(const Eigen::Isometry3d& vp, double out[7]) {
  const Eigen::Vector3d t = vp.translation();
  out[0] = t.x(); out[1] = t.y(); out[2] = t.z();
  rotationToQuaternion(vp.rotation(), out + 3);
}

// the data section at `body` into a cloud with the channels the header names
inline PointCloud decode(const fdm_pcd_header& h, const void* body, uint64_t body_bytes, PCDMetadata& meta_out) {
  meta_out.width = h.width;
  meta_out.height = h.height;
  meta_out.num_points = h.width * h.height;
  meta_out.viewpoint = Eigen::Isometry3d::Identity();
  meta_out.viewpoint.setTranslation(Eigen::Vector3d(h.viewpoint[0], h.viewpoint[1], h.viewpoint[2]));
  meta_out.viewpoint.setLinear(quaternionToRotation(h.viewpoint[3], h.viewpoint[4], h.viewpoint[5], h.viewpoint[6]));
  PointCloud cloud;
  if (meta_out.num_points == 0) return cloud;
  if (h.idx_intensity >= 0) cloud.useIntensity();
  if (h.idx_rgb >= 0) cloud.useColor();
  if (h.idx_nx >= 0 && h.idx_ny >= 0 && h.idx_nz >= 0) cloud.useNormal();
  cloud.resize(meta_out.num_points);
  const int rc = fdm_pcd_decode(&h, body, body_bytes, 0, cloud.xData(), cloud.yData(), cloud.zData(), cloud.intensityData(),
                                cloud.rgbData(), cloud.normalData(0), cloud.normalData(1), cloud.normalData(2), 0, 0);
  if (rc < 0) throw IOException(fdm_last_error());
  return cloud;
}

inline PointCloud loadBytes(const void* data, uint64_t n_bytes, PCDMetadata& meta_out) {
  fdm_pcd_header h;
  if (fdm_pcd_parse_header(data, n_bytes, &h) < 0) throw IOException(fdm_last_error());
  return decode(h, static_cast<const char*>(data) + h.data_offset, n_bytes - h.data_offset, meta_out);
}

// A PCD file as the device wants it: the header parsed from the file's first bytes, the data section read straight into
// a pinned block (fdm_host_alloc) of its own, so that it starts on a 16-byte boundary whatever the header's length and
// the decode kernel reads it in place with its widest loads.
struct PcdFile {
  fdm_pcd_header header;
  void* body = nullptr;
  uint64_t body_bytes = 0;
  PcdFile() = default;
  PcdFile(const PcdFile&) = delete;
  PcdFile& operator=(const PcdFile&) = delete;
  ~PcdFile() { fdm_host_free(body); }
};

inline void readFile(const std::string& path, PcdFile& f) {
  std::ifstream ifs(path, std::ios::binary | std::ios::ate);
  if (!ifs) throw IOException("Cannot open file: " + path);
  const std::streamoff end = ifs.tellg();
  if (end < 0) throw IOException("Cannot read file: " + path);
  const uint64_t size = uint64_t(end);
  std::string head;
  for (uint64_t prefix = 4096;; prefix *= 16) {  // the header: a few hundred bytes; more only if DATA is not in reach
    const uint64_t len = prefix < size ? prefix : size;
    head.resize(size_t(len));
    ifs.clear();
    ifs.seekg(0);
    if (len && !ifs.read(&head[0], std::streamsize(len))) throw IOException("Cannot read file: " + path);
    const int rc = fdm_pcd_parse_header(head.data(), len, &f.header);
    if (rc == 0 && (f.header.data_offset < len || len == size)) break;  // the DATA line lies inside what was read
    if (len == size) throw IOException(fdm_last_error());
  }
  f.body_bytes = size - f.header.data_offset;
  f.body = fdm_host_alloc(f.body_bytes ? f.body_bytes : 1);
  if (!f.body) throw IOException("Cannot allocate memory for file: " + path);
  ifs.clear();
  ifs.seekg(std::streamoff(f.header.data_offset));
  if (f.body_bytes && !ifs.read(static_cast<char*>(f.body), std::streamsize(f.body_bytes)))
    throw IOException("Cannot read file: " + path);
}

}  // namespace detail

/// Load a PCD file from a stream, from its current position to its end
inline PointCloud loadPCD(std::istream& is, PCDMetadata& meta_out) {
  if (!is) throw IOException("Invalid input stream");
  const std::string data((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
  return detail::loadBytes(data.data(), data.size(), meta_out);
}

/// Load a PCD file with its metadata
inline PointCloud loadPCD(const std::string& path, PCDMetadata& meta_out) {
  detail::PcdFile file;
  detail::readFile(path, file);
  return detail::decode(file.header, file.body, file.body_bytes, meta_out);
}

inline PointCloud loadPCD(const std::string& path) {
  PCDMetadata meta;
  return loadPCD(path, meta);
}

/// Save a cloud to a stream
inline void savePCD(std::ostream& os, const PointCloud& cloud, const PCDSaveOptions& options) {
  if (!os) throw IOException("Invalid output stream");
  const uint64_t n = cloud.size();
  const int format = options.format == PCDFormat::ASCII ? FDM_PCD_ASCII : FDM_PCD_BINARY;
  double vp[7];
  detail::viewpointNumbers(options.viewpoint, vp);
  char head[512];
  uint64_t head_bytes = 0;
  if (fdm_pcd_write_header(n, cloud.hasIntensity(), cloud.hasColor(), cloud.hasNormal(), vp, format, head, sizeof(head),
                           &head_bytes) != 0)
    throw IOException(std::string("fdm_pcd_write_header: ") + fdm_last_error());
  os.write(head, std::streamsize(head_bytes));
  std::vector<char> body(format == FDM_PCD_BINARY ? size_t(n) * 32 : 0);
  uint64_t body_bytes = 0;
  auto encode = [&] {
    return fdm_pcd_encode(n, cloud.xData(), cloud.yData(), cloud.zData(), cloud.intensityData(), cloud.rgbData(),
                          cloud.normalData(0), cloud.normalData(1), cloud.normalData(2), 0, format, options.precision, 0,
                          body.data(), body.size(), &body_bytes);
  };
  int rc = encode();
  if (rc > 0) {  // ASCII: the size is known once the text exists
    body.resize(size_t(body_bytes));
    rc = encode();
  }
  if (rc != 0) throw IOException(std::string("fdm_pcd_encode: ") + fdm_last_error());
  os.write(body.data(), std::streamsize(body_bytes));
  if (!os) throw IOException("Error writing PCD data");
}

/// Save a cloud to a file
inline void savePCD(const std::string& path, const PointCloud& cloud, const PCDSaveOptions& options = PCDSaveOptions()) {
  std::ofstream ofs(path, std::ios::binary);
  if (!ofs) throw IOException("Cannot create file: " + path);
  savePCD(ofs, cloud, options);
}

inline void savePCD(const std::string& path, const PointCloud& cloud, PCDFormat format) {
  PCDSaveOptions options;
  options.format = format;
  savePCD(path, cloud, options);
}

}  // namespace io
}  // namespace nanopcl
