// fdm_engine_ray.hip — the raycasting stage of one scan: voxel filter, stable radix sort, ray queue,
// the walks (fdm_raycast.hpp, fdm_raywedge.hpp, fdm_rsort.hpp), resolve; entry points fdm_engine_apply_raycasting*,
// fdm_engine_voxel_any, fdm_engine_last_ray_ms; and, on the same keys and sorts, the cloud downsampling filters
// (fdm_voxel.hpp; fdm_cloud_voxel_grid, fdm_cloud_grid_max_z).  One of the library's five translation units
// (fdm_engine_host.hpp).
#include "fdm_engine_host.hpp"

#include "fdm_engine_ray.inl"
#include "fdm_engine_voxel.inl"
