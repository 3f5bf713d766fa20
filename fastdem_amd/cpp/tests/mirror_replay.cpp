// mirror_replay — runs a script of map / mapper / layer-access steps through the C++ host mirror's public API
// (fastdem::FastDEM, ElevationMap, nanogrid::GridMap, ElevationMapping, postprocess/*.hpp) and writes what the test
// compares with the oracle running the same script (tests/mirror_script.py, tests/test_cpp_mirror_gpu.py).
//
//   mirror_replay <dir>      reads <dir>/script.txt and the blobs it names, writes <dir>/out/
//
// One step per line: an op and its whitespace-separated arguments.  Every returned bool, every lastStats() and every
// dump goes to out/log.txt; a dump's arrays go to out/dump_<k>.f32, callback clouds to out/cb_<k>.f32.  The binary
// reads nothing but <dir>.  Any exception ends the run with a non-zero status and the failing step on stderr.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "fastdem/fastdem.hpp"
#include "fastdem/postprocess/feature_extraction.hpp"
#include "fastdem/postprocess/inpainting.hpp"
#include "fastdem/postprocess/spatial_smoothing.hpp"
#include "fastdem/postprocess/uncertainty_fusion.hpp"

using namespace fastdem;

namespace {

// a user SensorModel subclass: the built-in LiDAR model's covariance, evaluated on the host (builtin() == false)
class HostLiDAR : public SensorModel {
 public:
  HostLiDAR(float range_noise, float angular_noise) : m_(range_noise, angular_noise) {}
  Eigen::Matrix3f computeCovariance(const Eigen::Vector3f& p) const override { return m_.computeCovariance(p); }

 private:
  LiDARSensorModel m_;
};

// sensor_msgs/PointCloud2 as integrateCloud2 reads it
struct Cloud2Msg {
  struct Field {
    std::string name;
    uint32_t offset;
    uint8_t datatype;
  };
  uint32_t width = 0, height = 1, point_step = 0;
  std::vector<uint8_t> data;
  std::vector<Field> fields;
};

struct Cloud {
  PointCloud soa;
  std::unique_ptr<nanopcl::PointCloud4> aos;
};

struct Handle {
  std::string slot, layer;
  nanogrid::Matrix* m;
};

struct Mapper {
  std::string slot;
  std::unique_ptr<FastDEM> fd;
  std::unique_ptr<ElevationMapping> em;
};

class Replay {
 public:
  explicit Replay(const std::string& dir) : dir_(dir), out_(dir + "/out") {
    log_ = std::fopen((out_ + "/log.txt").c_str(), "w");
    if (!log_) throw std::runtime_error("cannot write " + out_ + "/log.txt");
  }
  ~Replay() {
    mappers_.clear();  // (before the maps they are bound to)
    if (log_) std::fclose(log_);
  }

  void run() {
    std::ifstream in(dir_ + "/script.txt");
    if (!in) throw std::runtime_error("cannot read " + dir_ + "/script.txt");
    std::string line;
    int step = 0;
    while (std::getline(in, line)) {
      if (line.empty() || line[0] == '#') continue;
      std::istringstream ts(line);
      std::vector<std::string> t;
      for (std::string w; ts >> w;) t.push_back(w);
      try {
        exec(step, t);
      } catch (const std::exception& e) {
        throw std::runtime_error("step " + std::to_string(step) + " (" + line + "): " + e.what());
      }
      ++step;
    }
    std::fprintf(log_, "end %d\n", step);
  }

 private:
  // ---- helpers ----
  static float F(const std::string& s) { return std::strtof(s.c_str(), nullptr); }
  static double D(const std::string& s) { return std::strtod(s.c_str(), nullptr); }
  static int I(const std::string& s) { return std::atoi(s.c_str()); }
  std::vector<char> blob(const std::string& name) const {
    std::ifstream f(dir_ + "/" + name, std::ios::binary);
    if (!f) throw std::runtime_error("cannot read blob " + name);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  }
  ElevationMap& map(const std::string& s) {
    auto it = maps_.find(s);
    if (it == maps_.end()) throw std::runtime_error("no map slot " + s);
    return *it->second;
  }
  Mapper& mapper(const std::string& m) {
    auto it = mappers_.find(m);
    if (it == mappers_.end()) throw std::runtime_error("no mapper " + m);
    return it->second;
  }
  FastDEM& fd(const std::string& m) {
    Mapper& x = mapper(m);
    if (!x.fd) throw std::runtime_error(m + " is not a FastDEM");
    return *x.fd;
  }
  Cloud& cloud(const std::string& c) {
    auto it = clouds_.find(c);
    if (it == clouds_.end()) throw std::runtime_error("no cloud " + c);
    return it->second;
  }
  const Eigen::Isometry3d& pose(const std::string& p) {
    auto it = poses_.find(p);
    if (it == poses_.end()) throw std::runtime_error("no pose " + p);
    return it->second;
  }
  nanogrid::Matrix& handle(const std::string& h) {
    auto it = handles_.find(h);
    if (it == handles_.end()) throw std::runtime_error("no handle " + h);
    return *it->second.m;
  }
  void options(ElevationMap& m) {
    for (const auto& kv : options_)
      detail::ck(fdm_engine_set_option(m.engine(), kv.first.c_str(), kv.second), "fdm_engine_set_option");
  }
  // a slot's map goes away: first the mappers bound to it, then the handles into it
  void dropMappers(const std::string& s) {
    for (auto it = mappers_.begin(); it != mappers_.end();)
      it = it->second.slot == s ? mappers_.erase(it) : std::next(it);
  }
  void dropHandles(const std::string& s) {
    for (auto it = handles_.begin(); it != handles_.end();)
      it = it->second.slot == s ? handles_.erase(it) : std::next(it);
  }
  void ret(int step, const std::string& what, bool r, const fdm_scan_stats* st) {
    std::fprintf(log_, "ret %d %s %d", step, what.c_str(), r ? 1 : 0);
    if (st)
      std::fprintf(log_, " %u %u %u %u %d %d", st->n_input, st->n_after_filter, st->n_in_map, st->n_cells_touched,
                   st->shift_rows, st->shift_cols);
    std::fprintf(log_, "\n");
  }
  void writeF32(const std::string& file, const float* p, size_t n, bool append) {
    std::FILE* f = std::fopen((out_ + "/" + file).c_str(), append ? "ab" : "wb");
    if (!f || std::fwrite(p, sizeof(float), n, f) != n) throw std::runtime_error("cannot write " + file);
    std::fclose(f);
  }
  void cbRecord(const std::string& kind, const PointCloud& c) {
    const int k = ncb_++;
    const std::string file = "cb_" + std::to_string(k) + ".f32";
    std::vector<float> v;
    v.insert(v.end(), c.xData(), c.xData() + c.size());
    v.insert(v.end(), c.yData(), c.yData() + c.size());
    v.insert(v.end(), c.zData(), c.zData() + c.size());
    if (c.hasCovariance()) {
      const float* cov = const_cast<PointCloud&>(c).covarianceData();
      v.insert(v.end(), cov, cov + c.size() * 9);
    }
    writeF32(file, v.data(), v.size(), false);
    std::fprintf(log_, "cb %d %s %zu %d\n", k, kind.c_str(), c.size(), c.hasCovariance() ? 1 : 0);
  }
  void dump(int step, const std::string& s) {
    const ElevationMap& m = map(s);  // (const access: a dump marks nothing host-dirty)
    const int k = ndump_++;
    const std::string file = "dump_" + std::to_string(k) + ".f32";
    const nanogrid::Index st = m.getStartIndex();
    const nanogrid::Position pos = m.getPosition();
    const nanogrid::Size sz = m.getSize();
    std::fprintf(log_, "dump %d %d %s %d %d %d %d %.17g %.17g\n", step, k, s.c_str(), sz(0), sz(1), st(0), st(1),
                 pos(0), pos(1));
    std::FILE* f = std::fopen((out_ + "/" + file).c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + file);
    for (const auto& name : m.getLayers()) {  // every layer by a fresh get(), column-major as the mirror holds it
      const nanogrid::Matrix& a = m.get(name);
      std::fwrite(a.data(), sizeof(float), a.size(), f);
      std::fprintf(log_, "layer %s\n", name.c_str());
    }
    for (const auto& kv : handles_) {  // then every live handle of this map, read through the held reference
      if (kv.second.slot != s) continue;
      const nanogrid::Matrix& a = *kv.second.m;
      std::fwrite(a.data(), sizeof(float), a.size(), f);
      std::fprintf(log_, "handle %s %s\n", kv.first.c_str(), kv.second.layer.c_str());
    }
    std::fclose(f);
    std::fprintf(log_, "enddump\n");
  }

  void exec(int step, const std::vector<std::string>& t) {
    const std::string& op = t.at(0);
    auto a = [&](size_t i) -> const std::string& { return t.at(i); };
    // ---- inputs ----
    if (op == "option") {                       // option KEY VALUE: every engine created from here on
      options_[a(1)] = I(a(2));
    } else if (op == "pose") {                  // pose NAME m00 m01 ... m33 (row-major 4x4)
      Eigen::Isometry3d T = Eigen::Isometry3d::Identity();
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T.data()[c * 4 + r] = D(a(2 + size_t(r) * 4 + size_t(c)));
      poses_[a(1)] = T;
    } else if (op == "cloud") {                 // cloud NAME N HAS_INTENSITY HAS_RGB: NAME.xyz.f32 [NAME.i.f32] [NAME.rgb.u32]
      const size_t n = size_t(std::stoull(a(2)));
      const bool hi = I(a(3)), hc = I(a(4));
      Cloud& c = clouds_[a(1)];
      c.soa = PointCloud();
      c.aos.reset();
      if (n == 0) return;
      const std::vector<char> xyz = blob(a(1) + ".xyz.f32");
      if (xyz.size() != n * 12) throw std::runtime_error("bad xyz blob");
      const float* p = reinterpret_cast<const float*>(xyz.data());
      std::vector<char> ib, cb;
      if (hi) ib = blob(a(1) + ".i.f32");
      if (hc) cb = blob(a(1) + ".rgb.u32");
      c.soa.resize(n);
      if (hi) c.soa.useIntensity();
      if (hc) c.soa.useColor();
      for (size_t i = 0; i < n; ++i) {
        c.soa.point(i) = Eigen::Vector3f(p[i], p[n + i], p[2 * n + i]);
        if (hi) c.soa.intensity(i) = reinterpret_cast<const float*>(ib.data())[i];
        if (hc) {
          const uint32_t v = reinterpret_cast<const uint32_t*>(cb.data())[i];
          c.soa.setColor(i, nanopcl::Color(uint8_t(v >> 16), uint8_t(v >> 8), uint8_t(v)));
        }
      }
    // ---- maps ----
    } else if (op == "map") {                   // map S LX LY RES PX PY MOVE_CLEAR_BASIC
      dropMappers(a(1));
      dropHandles(a(1));
      auto m = std::make_unique<ElevationMap>();
      m->setMoveClearBasic(I(a(7)) != 0);
      m->setGeometry(F(a(2)), F(a(3)), F(a(4)));
      options(*m);
      m->setPosition(nanogrid::Position(D(a(5)), D(a(6))));
      maps_[a(1)] = std::move(m);
    } else if (op == "setpos") {
      map(a(1)).setPosition(nanogrid::Position(D(a(2)), D(a(3))));
    } else if (op == "setstart") {
      map(a(1)).setStartIndex(nanogrid::Index(I(a(2)), I(a(3))));
    } else if (op == "copy") {                  // copy DST SRC: copy construction
      ElevationMap& src = map(a(2));
      dropMappers(a(1));
      dropHandles(a(1));
      maps_[a(1)] = std::make_unique<ElevationMap>(src);
      options(*maps_[a(1)]);
    } else if (op == "copyassign") {            // copyassign DST SRC: DST exists; its mappers stay bound, its handles die
      ElevationMap& src = map(a(2));
      ElevationMap& dst = map(a(1));
      for (auto& kv : mappers_)
        if (kv.second.slot == a(1) && kv.second.fd) kv.second.fd->drain();
      dropHandles(a(1));
      dst = src;
      options(dst);
    } else if (op == "move" || op == "moveassign") {  // move DST SRC: std::move construction / assignment
      ElevationMap& src = map(a(2));
      for (auto& kv : mappers_)
        if (kv.second.slot == a(2) && kv.second.fd) kv.second.fd->drain();
      if (op == "move") {
        dropMappers(a(1));
        dropHandles(a(1));
        auto m = std::make_unique<ElevationMap>(std::move(src));
        dropMappers(a(2));
        maps_[a(1)] = std::move(m);
      } else {
        ElevationMap& dst = map(a(1));
        for (auto& kv : mappers_)
          if (kv.second.slot == a(1) && kv.second.fd) kv.second.fd->drain();
        dropMappers(a(1));
        dropHandles(a(1));
        dst = std::move(src);
        dropMappers(a(2));
      }
      maps_.erase(a(2));
      for (auto& kv : handles_)  // (a held reference keeps its address: it now reads the destination)
        if (kv.second.slot == a(2)) kv.second.slot = a(1);
    } else if (op == "snapshot") {              // snapshot DST SRC L1,L2,...
      std::vector<std::string> names;
      std::stringstream ss(a(3));
      for (std::string n; std::getline(ss, n, ',');) names.push_back(n);
      ElevationMap& src = map(a(2));
      ElevationMap snap;
      switch (names.size()) {  // (snapshot takes an initializer_list)
        case 1: snap = src.snapshot({names[0]}); break;
        case 2: snap = src.snapshot({names[0], names[1]}); break;
        case 3: snap = src.snapshot({names[0], names[1], names[2]}); break;
        case 4: snap = src.snapshot({names[0], names[1], names[2], names[3]}); break;
        default: throw std::runtime_error("snapshot takes 1-4 layers");
      }
      dropMappers(a(1));
      dropHandles(a(1));
      maps_[a(1)] = std::make_unique<ElevationMap>(std::move(snap));
      options(*maps_[a(1)]);
    } else if (op == "drop") {                  // drop S: the slot's mappers, handles and map go away
      dropMappers(a(1));
      dropHandles(a(1));
      maps_.erase(a(1));
    // ---- mappers ----
    } else if (op == "fastdem") {               // fastdem M S [YAML]
      Mapper x;
      x.slot = a(2);
      x.fd = t.size() > 3 ? std::make_unique<FastDEM>(map(a(2)), loadConfig(dir_ + "/" + a(3)))
                          : std::make_unique<FastDEM>(map(a(2)));
      mappers_.erase(a(1));
      mappers_[a(1)] = std::move(x);
    } else if (op == "emapping") {              // emapping M S MODE(local|global) EST(kalman|p2)
      config::Mapping c;
      c.mode = a(3) == "global" ? MappingMode::GLOBAL : MappingMode::LOCAL;
      c.estimation_type = a(4) == "p2" ? EstimationType::P2Quantile : EstimationType::Kalman;
      Mapper x;
      x.slot = a(2);
      x.em = std::make_unique<ElevationMapping>(map(a(2)), c);
      mappers_.erase(a(1));
      mappers_[a(1)] = std::move(x);
    } else if (op == "estimator") {
      fd(a(1)).setEstimatorType(a(2) == "p2" ? EstimationType::P2Quantile : EstimationType::Kalman);
    } else if (op == "sensor") {                // sensor M KIND [params]
      FastDEM& f = fd(a(1));
      if (a(2) == "constant") f.setSensorModel(std::make_unique<ConstantUncertaintyModel>(F(a(3))));
      else if (a(2) == "lidar") f.setSensorModel(std::make_unique<LiDARSensorModel>(F(a(3)), F(a(4))));
      else if (a(2) == "rgbd") f.setSensorModel(std::make_unique<RGBDSensorModel>(F(a(3)), F(a(4)), F(a(5)), F(a(6))));
      else if (a(2) == "hostlidar") f.setSensorModel(std::make_unique<HostLiDAR>(F(a(3)), F(a(4))));
      else if (a(2) == "type") f.setSensorModel(a(3) == "constant" ? SensorType::Constant
                                                : a(3) == "rgbd"   ? SensorType::RGBD
                                                                   : SensorType::LiDAR);
      else throw std::runtime_error("unknown sensor " + a(2));
    } else if (op == "height") {
      fd(a(1)).setHeightFilter(F(a(2)), F(a(3)));
    } else if (op == "range") {
      fd(a(1)).setRangeFilter(F(a(2)), F(a(3)));
    } else if (op == "mode") {
      fd(a(1)).setMappingMode(a(2) == "global" ? MappingMode::GLOBAL : MappingMode::LOCAL);
    } else if (op == "raycast") {
      fd(a(1)).enableRaycasting(I(a(2)) != 0);
    } else if (op == "queued") {
      fd(a(1)).setQueued(I(a(2)) != 0);
    } else if (op == "callbacks") {             // callbacks M ON: record both scan callbacks' clouds
      if (I(a(2))) {
        fd(a(1)).onScanPreprocessed([this](const PointCloud& c) { cbRecord("pre", c); });
        fd(a(1)).onScanRasterized([this](const PointCloud& c) { cbRecord("ras", c); });
      } else {
        fd(a(1)).onScanPreprocessed(nullptr);
        fd(a(1)).onScanRasterized(nullptr);
      }
    // ---- scans ----
    } else if (op == "integrate") {             // integrate M CLOUD TBS TWB
      FastDEM& f = fd(a(1));
      const bool r = f.integrate(cloud(a(2)).soa, pose(a(3)), pose(a(4)));
      ret(step, op, r, f.queued() ? nullptr : &f.lastStats());
    } else if (op == "integrate4") {
      FastDEM& f = fd(a(1));
      Cloud& c = cloud(a(2));
      if (!c.aos) {
        c.aos = std::make_unique<nanopcl::PointCloud4>();
        if (c.soa.hasIntensity()) c.aos->useIntensity();
        if (c.soa.hasColor()) c.aos->useColor();
        for (size_t i = 0; i < c.soa.size(); ++i) {
          const Eigen::Vector3f p = c.soa.point(i);
          if (c.soa.hasIntensity() && c.soa.hasColor())
            c.aos->add(p[0], p[1], p[2], nanopcl::Intensity(c.soa.intensity(i)), c.soa.color(i));
          else if (c.soa.hasIntensity()) c.aos->add(p[0], p[1], p[2], nanopcl::Intensity(c.soa.intensity(i)));
          else if (c.soa.hasColor()) c.aos->add(p[0], p[1], p[2], c.soa.color(i));
          else c.aos->add(p[0], p[1], p[2]);
        }
      }
      const bool r = f.integrate(*c.aos, pose(a(3)), pose(a(4)));
      ret(step, op, r, &f.lastStats());
    } else if (op == "batch") {                 // batch M CLOUD:TBS:TWB ...
      FastDEM& f = fd(a(1));
      std::vector<FastDEM::Scan> scans;
      for (size_t i = 2; i < t.size(); ++i) {
        std::stringstream ss(a(i));
        std::string c, tb, tw;
        std::getline(ss, c, ':');
        std::getline(ss, tb, ':');
        std::getline(ss, tw, ':');
        scans.push_back(FastDEM::Scan{&cloud(c).soa, pose(tb), pose(tw)});
      }
      const bool r = f.integrateBatch(scans);
      ret(step, op, r, &f.lastStats());
    } else if (op == "cloud2") {                // cloud2 M BLOB WIDTH POINT_STEP FIELD:OFFSET:TYPE,... TBS TWB
      FastDEM& f = fd(a(1));
      Cloud2Msg msg;
      const std::vector<char> b = blob(a(2));
      msg.data.assign(b.begin(), b.end());
      msg.width = uint32_t(std::stoul(a(3)));
      msg.point_step = uint32_t(std::stoul(a(4)));
      std::stringstream ss(a(5));
      for (std::string fld; std::getline(ss, fld, ',');) {
        const size_t p1 = fld.find(':'), p2 = fld.rfind(':');
        msg.fields.push_back({fld.substr(0, p1), uint32_t(std::stoul(fld.substr(p1 + 1, p2 - p1 - 1))),
                              uint8_t(std::stoul(fld.substr(p2 + 1)))});
      }
      const bool r = f.integrateCloud2(msg, pose(a(6)), pose(a(7)));
      ret(step, op, r, &f.lastStats());
    } else if (op == "drain") {
      FastDEM& f = fd(a(1));
      const bool r = f.drain();
      ret(step, op, r, &f.lastStats());
    } else if (op == "update") {                // update M CLOUD RX RY (ElevationMapping)
      Mapper& x = mapper(a(1));
      if (!x.em) throw std::runtime_error(a(1) + " is not an ElevationMapping");
      const auto o = x.em->update(cloud(a(2)).soa, Eigen::Vector2d(D(a(3)), D(a(4))));
      std::fprintf(log_, "ret %d update 1 %zu %zu\n", step, o.n_cells, o.n_points_in_map);
    // ---- layer access ----
    } else if (op == "touch") {                 // touch S LAYER: one host access (const: marks nothing)
      (void)static_cast<const ElevationMap&>(map(a(1))).get(a(2));
    } else if (op == "get") {                   // get H S LAYER: a handle kept across later steps
      handles_[a(1)] = Handle{a(2), a(3), &map(a(2)).get(a(3))};
    } else if (op == "hwrite") {                // hwrite H R C V
      handle(a(1))(I(a(2)), I(a(3))) = F(a(4));
    } else if (op == "hwritepos") {             // hwritepos H X Y V: the cell of (X, Y) in the handle's map
      nanogrid::Index i;
      if (!map(handles_.at(a(1)).slot).getIndex(nanogrid::Position(D(a(2)), D(a(3))), i))
        throw std::runtime_error("position outside the map");
      handle(a(1))(i) = F(a(4));
    } else if (op == "hfill") {               // hfill H V (setConstant through the handle)
      handle(a(1)).setConstant(F(a(2)));
    } else if (op == "hdata") {                 // hdata H K V: data()[K] = V through the handle
      handle(a(1)).data()[std::stoul(a(2))] = F(a(3));
    } else if (op == "at") {                    // at S LAYER R C V
      map(a(1)).at(a(2), nanogrid::Index(I(a(3)), I(a(4)))) = F(a(5));
    } else if (op == "atpos") {                 // atpos S LAYER X Y V
      map(a(1)).atPosition(a(2), nanogrid::Position(D(a(3)), D(a(4)))) = F(a(5));
    } else if (op == "clearat") {
      map(a(1)).clearAt(nanogrid::Index(I(a(2)), I(a(3))));
    } else if (op == "add") {                   // add S NAME [VALUE]
      if (t.size() > 3) map(a(1)).add(a(2), F(a(3)));
      else map(a(1)).add(a(2));
    } else if (op == "addm") {                  // addm S NAME BLOB (rows x cols floats, column-major)
      ElevationMap& m = map(a(1));
      const std::vector<char> b = blob(a(3));
      nanogrid::Matrix x(m.getSize()(0), m.getSize()(1));
      if (b.size() != x.size() * 4) throw std::runtime_error("bad matrix blob");
      std::memcpy(x.data(), b.data(), b.size());
      m.add(a(2), x);
    } else if (op == "clear") {
      map(a(1)).clear(a(2));
    } else if (op == "clearall") {
      map(a(1)).clearAll();
    } else if (op == "mapmove") {               // mapmove S X Y
      const bool r = map(a(1)).move(nanogrid::Position(D(a(2)), D(a(3))));
      ret(step, op, r, nullptr);
    // ---- stencils ----
    } else if (op == "inpaint") {               // inpaint S ITER MIN_VALID INPLACE
      applyInpainting(map(a(1)), I(a(2)), I(a(3)), I(a(4)) != 0);
    } else if (op == "smooth") {                // smooth S LAYER KERNEL MIN_VALID
      applySpatialSmoothing(map(a(1)), a(2), I(a(3)), I(a(4)));
    } else if (op == "fusion") {                // fusion S RADIUS SIGMA QLO QHI MIN_VALID
      config::UncertaintyFusion c;
      c.enabled = true;
      c.search_radius = F(a(2));
      c.spatial_sigma = F(a(3));
      c.quantile_lower = F(a(4));
      c.quantile_upper = F(a(5));
      c.min_valid_neighbors = I(a(6));
      applyUncertaintyFusion(map(a(1)), c);
    } else if (op == "features") {              // features S RADIUS MIN_VALID LO HI
      applyFeatureExtraction(map(a(1)), F(a(2)), I(a(3)), F(a(4)), F(a(5)));
    } else if (op == "raycasting") {            // raycasting S CLOUD OX OY OZ (config::Raycasting defaults)
      config::Raycasting c;
      c.enabled = true;
      applyRaycasting(map(a(1)), cloud(a(2)).soa, Eigen::Vector3f(F(a(3)), F(a(4)), F(a(5))), c);
    // ---- output ----
    } else if (op == "dump") {
      dump(step, a(1));
    } else {
      throw std::runtime_error("unknown op " + op);
    }
  }

  std::string dir_, out_;
  std::FILE* log_ = nullptr;
  std::map<std::string, int> options_;
  std::map<std::string, Eigen::Isometry3d> poses_;
  std::map<std::string, Cloud> clouds_;
  std::map<std::string, std::unique_ptr<ElevationMap>> maps_;
  std::map<std::string, Mapper> mappers_;
  std::map<std::string, Handle> handles_;
  int ndump_ = 0, ncb_ = 0;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <script dir>\n", argv[0]);
    return 2;
  }
  try {
    Replay r(argv[1]);
    r.run();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mirror_replay: %s\n", e.what());
    return 1;
  }
  return 0;
}
