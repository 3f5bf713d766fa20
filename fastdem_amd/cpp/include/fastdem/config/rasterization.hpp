// fastdem/config/rasterization.hpp — how fromPointCloud() picks a cell's elevation
// (fastdem/include/fastdem/config/rasterization.hpp).  The enumerators' values are the engine's `method` argument.
#pragma once

namespace fastdem {

enum class RasterMethod {
  Max,     // the highest z of the cell
  Min,     // the lowest
  Mean,    // Welford's running mean, in input order
  MinMax,  // elevation = the highest; elevation_min / elevation_max carry both ends (as they always do)
};

namespace config {
struct Rasterization {
  RasterMethod method = RasterMethod::Max;
};
}  // namespace config

}  // namespace fastdem
