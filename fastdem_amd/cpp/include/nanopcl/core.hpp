// nanopcl/core.hpp — the nanopcl::PointCloud surface FastDEM::integrate() consumes
// (fastdem/lib/nanoPCL/include/nanopcl/core/point_cloud.hpp:24-147, types.hpp), re-laid out as
// SoA channels: x / y / z / intensity / packed rgb are separate contiguous float arrays, which is
// exactly what the engine's C ABI takes — no AoS->SoA staging pass on the host.  The channels live in
// pinned memory from the engine's pool (fdm_host_alloc), so FastDEM::integrate() reads a cloud in
// place over PCIe instead of copying it first.
#pragma once
#include <cstddef>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "fastdem/compat/mini_eigen.hpp"
#include "fdm_engine.h"

namespace nanopcl {

// std::allocator over fdm_host_alloc / fdm_host_free (a free-list pop per cloud, not a driver call)
template <typename T>
struct HostAllocator {
  using value_type = T;
  HostAllocator() = default;
  template <typename U>
  HostAllocator(const HostAllocator<U>&) {}
  T* allocate(std::size_t n) {
    void* p = fdm_host_alloc(uint64_t(n) * sizeof(T));
    if (!p) throw std::bad_alloc();
    return static_cast<T*>(p);
  }
  void deallocate(T* p, std::size_t) { fdm_host_free(p); }
  template <typename U>
  bool operator==(const HostAllocator<U>&) const { return true; }
  template <typename U>
  bool operator!=(const HostAllocator<U>&) const { return false; }
};
template <typename T>
using HostVector = std::vector<T, HostAllocator<T>>;

using Point = Eigen::Vector3f;

struct Intensity {
  float val;
  explicit constexpr Intensity(float v = 0.0f) : val(v) {}
  constexpr operator float() const { return val; }
};

struct Color {
  uint8_t r, g, b;
  constexpr Color() : r(0), g(0), b(0) {}
  constexpr Color(uint8_t r_, uint8_t g_, uint8_t b_) : r(r_), g(g_), b(b_) {}
};

struct Label {  // upper 16 bits: semantic class, lower 16 bits: instance id
  uint32_t val;
  constexpr Label() : val(0) {}
  explicit constexpr Label(uint32_t v) : val(v) {}
  constexpr operator uint32_t() const { return val; }
  constexpr uint16_t semanticClass() const { return uint16_t(val >> 16); }
  constexpr uint16_t instanceId() const { return uint16_t(val & 0xFFFFu); }
};

// core/span.hpp: a view over contiguous elements (what ClusterResult::clusterIndices hands out)
template <typename T>
class Span {
 public:
  constexpr Span() noexcept : data_(nullptr), size_(0) {}
  constexpr Span(T* data, size_t size) noexcept : data_(data), size_(size) {}
  constexpr T* data() const noexcept { return data_; }
  constexpr size_t size() const noexcept { return size_; }
  constexpr bool empty() const noexcept { return size_ == 0; }
  constexpr T& operator[](size_t i) const { return data_[i]; }
  constexpr T* begin() const noexcept { return data_; }
  constexpr T* end() const noexcept { return data_ + size_; }
  constexpr T& front() const { return data_[0]; }
  constexpr T& back() const { return data_[size_ - 1]; }

 private:
  T* data_;
  size_t size_;
};

// core/types.hpp:19-22 — Eigen::Vector4f there; the same 16 bytes here
struct alignas(16) Point4 {
  float v[4];
  constexpr Point4() : v{0.0f, 0.0f, 0.0f, 0.0f} {}
  constexpr Point4(float x, float y, float z, float w) : v{x, y, z, w} {}
  float& x() { return v[0]; }
  float& y() { return v[1]; }
  float& z() { return v[2]; }
  float& w() { return v[3]; }
  float x() const { return v[0]; }
  float y() const { return v[1]; }
  float z() const { return v[2]; }
  float w() const { return v[3]; }
  float& operator[](int i) { return v[size_t(i)]; }
  float operator[](int i) const { return v[size_t(i)]; }
  float* data() { return v; }
  const float* data() const { return v; }
};
using Normal4 = Point4;  // a normal's fourth component is 0; the SoA cloud keeps x, y, z

class PointCloud {
 public:
  // xyz view of one point (reads and writes go to the SoA channels)
  struct PointRef {
    float &x_, &y_, &z_;
    float x() const { return x_; }
    float y() const { return y_; }
    float z() const { return z_; }
    PointRef& operator=(const Eigen::Vector3f& p) { x_ = p[0]; y_ = p[1]; z_ = p[2]; return *this; }
    operator Eigen::Vector3f() const { return Eigen::Vector3f(x_, y_, z_); }
  };

  // one point's normal in the SoA channels, and the channel as a sequence (normals()[i], normals().back())
  struct NormalRef {
    float &x_, &y_, &z_;
    float x() const { return x_; }
    float y() const { return y_; }
    float z() const { return z_; }
    float w() const { return 0.0f; }
    NormalRef& operator=(const Normal4& n) { x_ = n.x(); y_ = n.y(); z_ = n.z(); return *this; }
    operator Normal4() const { return Normal4(x_, y_, z_, 0.0f); }
  };
  struct NormalsView {
    PointCloud* cloud;
    size_t size() const { return cloud->nx_.size(); }
    NormalRef operator[](size_t i) const { return NormalRef{cloud->nx_[i], cloud->ny_[i], cloud->nz_[i]}; }
    NormalRef back() const { return (*this)[size() - 1]; }
  };

  PointCloud() = default;
  explicit PointCloud(size_t n) { resize(n); }

  size_t size() const { return x_.size(); }
  bool empty() const { return x_.empty(); }
  void reserve(size_t n) { x_.reserve(n); y_.reserve(n); z_.reserve(n); }
  void resize(size_t n) {
    x_.resize(n); y_.resize(n); z_.resize(n);
    if (use_intensity_) intensity_.resize(n);
    if (use_color_) rgb_.resize(n);
    if (use_normal_) { nx_.resize(n); ny_.resize(n); nz_.resize(n); }
    if (use_cov_) cov_.resize(n * 9);
    if (use_label_) label_.resize(n);
  }
  void clear() { resize(0); }

  void add(float x, float y, float z) {
    x_.push_back(x); y_.push_back(y); z_.push_back(z);
    if (use_intensity_) intensity_.push_back(0.0f);
    if (use_color_) rgb_.push_back(0u);
    if (use_normal_) { nx_.push_back(0.0f); ny_.push_back(0.0f); nz_.push_back(0.0f); }
    if (use_cov_) cov_.resize(cov_.size() + 9, 0.0f);
    if (use_label_) label_.push_back(Label());
  }
  void add(float x, float y, float z, Intensity i) {
    if (!use_intensity_) useIntensity();
    add(x, y, z);
    intensity_.back() = i.val;
  }
  void add(float x, float y, float z, const Color& c) {
    if (!use_color_) useColor();
    add(x, y, z);
    rgb_.back() = pack(c);
  }

  PointRef point(size_t i) { return PointRef{x_[i], y_[i], z_[i]}; }
  Eigen::Vector3f point(size_t i) const { return Eigen::Vector3f(x_[i], y_[i], z_[i]); }

  bool hasIntensity() const { return use_intensity_; }
  void useIntensity() { use_intensity_ = true; intensity_.resize(size(), 0.0f); }
  float& intensity(size_t i) { return intensity_[i]; }
  float intensity(size_t i) const { return intensity_[i]; }

  // covariance channel (nanopcl/core/point_cloud.hpp:126-147): the cloud the preprocessed-scan callback
  // receives carries R * Sigma_sensor * R^T per point
  bool hasCovariance() const { return use_cov_; }
  void useCovariance() { use_cov_ = true; cov_.resize(size() * 9, 0.0f); }
  Eigen::Matrix3f covariance(size_t i) const {
    Eigen::Matrix3f m;
    for (int c = 0; c < 3; ++c)
      for (int r = 0; r < 3; ++r) m(r, c) = cov_[i * 9 + size_t(c) * 3 + size_t(r)];
    return m;
  }
  float* covarianceData() { return use_cov_ ? cov_.data() : nullptr; }  // [n][9], column-major 3x3 per point
  const float* covarianceData() const { return use_cov_ ? cov_.data() : nullptr; }

  bool hasColor() const { return use_color_; }
  void useColor() { use_color_ = true; rgb_.resize(size(), 0u); }
  Color color(size_t i) const { return Color(uint8_t(rgb_[i] >> 16), uint8_t(rgb_[i] >> 8), uint8_t(rgb_[i])); }
  void setColor(size_t i, const Color& c) { rgb_[i] = pack(c); }

  // normal channel (nanopcl/core/point_cloud.hpp): what loadPCD fills from normal_x / normal_y / normal_z
  bool hasNormal() const { return use_normal_; }
  void useNormal() { use_normal_ = true; nx_.resize(size(), 0.0f); ny_.resize(size(), 0.0f); nz_.resize(size(), 0.0f); }
  Normal4 normal(size_t i) const { return Normal4(nx_[i], ny_[i], nz_[i], 0.0f); }
  NormalRef normal(size_t i) { return NormalRef{nx_[i], ny_[i], nz_[i]}; }
  NormalsView normals() { return NormalsView{this}; }

  // label channel (nanopcl/core/point_cloud.hpp): what applyClusterLabels writes
  bool hasLabel() const { return use_label_; }
  void useLabel() { use_label_ = true; label_.resize(size(), Label()); }
  std::vector<Label>& labels() { return label_; }
  const std::vector<Label>& labels() const { return label_; }
  Label& label(size_t i) { return label_[i]; }
  const Label& label(size_t i) const { return label_[i]; }

  // the listed points, in list order, with every channel this cloud carries and its metadata
  // (core/impl/point_cloud_impl.hpp:176-216)
  PointCloud extract(const std::vector<size_t>& idx) const {
    PointCloud out;
    out.frame_id_ = frame_id_;
    out.timestamp_ns_ = timestamp_ns_;
    if (use_intensity_) out.useIntensity();
    if (use_color_) out.useColor();
    if (use_normal_) out.useNormal();
    if (use_cov_) out.useCovariance();
    if (use_label_) out.useLabel();
    out.resize(idx.size());
    for (size_t k = 0; k < idx.size(); ++k) {
      const size_t i = idx[k];
      out.x_[k] = x_[i]; out.y_[k] = y_[i]; out.z_[k] = z_[i];
      if (use_intensity_) out.intensity_[k] = intensity_[i];
      if (use_color_) out.rgb_[k] = rgb_[i];
      if (use_normal_) { out.nx_[k] = nx_[i]; out.ny_[k] = ny_[i]; out.nz_[k] = nz_[i]; }
      if (use_cov_) for (size_t q = 0; q < 9; ++q) out.cov_[k * 9 + q] = cov_[i * 9 + q];
      if (use_label_) out.label_[k] = label_[i];
    }
    return out;
  }

  const std::string& frameId() const { return frame_id_; }
  void setFrameId(const std::string& id) { frame_id_ = id; }
  uint64_t timestamp() const { return timestamp_ns_; }
  void setTimestamp(uint64_t ns) { timestamp_ns_ = ns; }

  // SoA channel access (what the C ABI binds)
  const float* xData() const { return x_.data(); }
  const float* yData() const { return y_.data(); }
  const float* zData() const { return z_.data(); }
  const float* intensityData() const { return use_intensity_ ? intensity_.data() : nullptr; }
  const uint32_t* rgbData() const { return use_color_ ? rgb_.data() : nullptr; }
  const float* normalData(int axis) const { return !use_normal_ ? nullptr : (axis == 0 ? nx_ : (axis == 1 ? ny_ : nz_)).data(); }
  // ... and for the calls that fill a cloud in place (loadPCD)
  float* xData() { return x_.data(); }
  float* yData() { return y_.data(); }
  float* zData() { return z_.data(); }
  float* intensityData() { return use_intensity_ ? intensity_.data() : nullptr; }
  uint32_t* rgbData() { return use_color_ ? rgb_.data() : nullptr; }
  float* normalData(int axis) { return !use_normal_ ? nullptr : (axis == 0 ? nx_ : (axis == 1 ? ny_ : nz_)).data(); }

 private:
  static uint32_t pack(const Color& c) { return (uint32_t(c.r) << 16) | (uint32_t(c.g) << 8) | uint32_t(c.b); }
  HostVector<float> x_, y_, z_, intensity_, nx_, ny_, nz_;
  HostVector<uint32_t> rgb_;  // 0x00RRGGBB
  std::vector<float> cov_;
  std::vector<Label> label_;
  std::string frame_id_;
  uint64_t timestamp_ns_ = 0;
  bool use_intensity_ = false, use_color_ = false, use_cov_ = false, use_normal_ = false, use_label_ = false;
};

}  // namespace nanopcl

#include "nanopcl/geometry/normal_estimation.hpp"  // estimateNormals, estimateCovariances, estimateNormalsCovariances
#include "nanopcl/registration.hpp"                // alignICP, alignPlaneICP, alignGICP
#include "nanopcl/segmentation.hpp"                // segmentGround, segmentPlane(s), euclideanCluster, applyClusterLabels
