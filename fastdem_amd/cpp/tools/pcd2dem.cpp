// pcd2dem — convert a PCD point cloud map to a clean elevation map, on the device: the reference's fastdem/tools/pcd2dem.cpp
// (loadPCD -> buildDEM -> toPointCloud -> savePCD) with its command line and console lines.  The file's records are read
// into pinned memory on a 16-byte boundary, decoded on the device straight into buildDEM's input (fdm_pcd_build_dem),
// and the map leaves as savePCD's records (fdm_engine_to_pcd): the cloud never exists on the host as arrays.
//
// Usage:
//   ./pcd2dem input.pcd output.pcd [resolution]
#include <cstdint>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "fdm_engine.h"
#include "nanopcl/io/pcd_io.hpp"

namespace {
int fail(const std::string& what) {
  std::cerr << "pcd2dem: " << what << std::endl;
  return 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "Usage: pcd2dem <input.pcd> <output.pcd> [resolution]\n"
              << "  resolution: grid cell size in meters (default: 0.1)\n";
    return 1;
  }
  const std::string input_path = argv[1];
  const std::string output_path = argv[2];
  fdm_dem_config config;
  fdm_default_dem_config(&config);
  if (argc >= 4) config.resolution = std::stof(argv[3]);

  // Load
  std::cout << "Loading " << input_path << " ..." << std::endl;
  nanopcl::io::detail::PcdFile file;  // the header, and the records in pinned memory on a 16-byte boundary
  try {
    nanopcl::io::detail::readFile(input_path, file);
  } catch (const nanopcl::io::IOException& e) {
    return fail(e.what());
  }
  const fdm_pcd_header& header = file.header;
  std::cout << "  " << header.width * header.height << " points" << std::endl;

  // Build DEM (SOR -> histogram filter -> rasterize -> inpaint)
  std::cout << "Building DEM (resolution=" << config.resolution << "m) ..." << std::endl;
  fdm_engine* dem = nullptr;
  const int rc = fdm_pcd_build_dem(&header, file.body, file.body_bytes, 0, &config, 0, &dem, nullptr);
  if (rc < 0) return fail(fdm_last_error());
  fdm_geometry g{};
  if (dem && fdm_engine_get_geometry(dem, &g) < 0) {
    fdm_engine_destroy(dem);
    return fail(fdm_last_error());
  }
  std::cout << "  Grid: " << g.rows << " x " << g.cols << " cells" << std::endl;

  // Export (a cloud that leaves no map gives a file of 0 points)
  std::vector<char> body(size_t(g.rows) * size_t(g.cols) * 20);
  uint64_t body_bytes = 0, n = 0;
  int32_t has_intensity = 0, has_color = 0;
  if (dem) {
    const int rc_out = fdm_engine_to_pcd(dem, body.data(), body.size(), &body_bytes, &n, &has_intensity, &has_color);
    fdm_engine_destroy(dem);
    if (rc_out != 0) return fail(rc_out < 0 ? fdm_last_error() : "the map does not fit the output buffer");
  }
  std::cout << "  " << n << " elevation cells" << std::endl;
  char head[512];
  uint64_t head_bytes = 0;
  if (fdm_pcd_write_header(n, has_intensity, has_color, 0, nullptr, FDM_PCD_BINARY, head, sizeof(head), &head_bytes) != 0)
    return fail(fdm_last_error());
  std::ofstream ofs(output_path, std::ios::binary);
  if (!ofs) return fail("Cannot create file: " + output_path);
  ofs.write(head, std::streamsize(head_bytes));
  ofs.write(body.data(), std::streamsize(body_bytes));
  if (!ofs) return fail("Error writing PCD data");
  std::cout << "Saved to " << output_path << std::endl;
  return 0;
}
