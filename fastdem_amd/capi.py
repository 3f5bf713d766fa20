"""ctypes declarations for include/fdm_engine.h (libfdm_engine.so).

Plumbing only: the product is the HIP library.  Loading fails loudly when the library
has not been built — there is no Python or CPU fallback for any entry point.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfdm_engine.so")  # (measurement scripts assign another build of the same ABI here before load())


class FdmConfig(C.Structure):
    """fdm_config == fastdem::Config for this path (config/fastdem.hpp:23-38)."""

    _fields_ = [
        ("z_min", C.c_float), ("z_max", C.c_float),
        ("range_min", C.c_float), ("range_max", C.c_float),
        ("sensor_type", C.c_int32),
        ("lidar_range_noise", C.c_float), ("lidar_angular_noise", C.c_float),
        ("rgbd_normal_a", C.c_float), ("rgbd_normal_b", C.c_float),
        ("rgbd_normal_c", C.c_float), ("rgbd_lateral_factor", C.c_float),
        ("constant_uncertainty", C.c_float),
        ("mode", C.c_int32), ("estimation_type", C.c_int32),
        ("kalman_min_variance", C.c_float), ("kalman_max_variance", C.c_float),
        ("kalman_process_noise", C.c_float),
        ("p2_dn", C.c_float * 5),
        ("p2_elevation_marker", C.c_int32),
        ("p2_max_sample_count", C.c_float),
        # config::Raycasting (config/postprocess.hpp:16-23)
        ("raycast_enabled", C.c_int32),
        ("rc_height_conflict_threshold", C.c_float), ("rc_log_odds_observed", C.c_float),
        ("rc_log_odds_ghost", C.c_float), ("rc_log_odds_max", C.c_float),
        ("rc_clear_threshold", C.c_float),
    ]


class FdmRaycastConfig(C.Structure):
    """fdm_raycast_config == config::Raycasting (config/postprocess.hpp:16-23)."""

    _fields_ = [
        ("enabled", C.c_int32),
        ("height_conflict_threshold", C.c_float), ("log_odds_observed", C.c_float),
        ("log_odds_ghost", C.c_float), ("log_odds_max", C.c_float), ("clear_threshold", C.c_float),
    ]


class FdmCloud2Layout(C.Structure):
    """fdm_cloud2_layout: byte offsets of the PointCloud2 fields integrate() consumes (-1 = absent)."""

    _fields_ = [
        ("point_step", C.c_uint32),
        ("off_x", C.c_int32), ("off_y", C.c_int32), ("off_z", C.c_int32),
        ("off_intensity", C.c_int32), ("intensity_type", C.c_int32),
        ("off_rgb", C.c_int32),
    ]


class FdmFusionConfig(C.Structure):
    """fdm_fusion_config == config::UncertaintyFusion (config/postprocess.hpp:32-39)."""

    _fields_ = [
        ("enabled", C.c_int32),
        ("search_radius", C.c_float), ("spatial_sigma", C.c_float),
        ("quantile_lower", C.c_float), ("quantile_upper", C.c_float),
        ("min_valid_neighbors", C.c_int32),
    ]


class FdmImageConfig(C.Structure):
    """fdm_image_config == fastdem::io::PngExportConfig (io/png.hpp)."""

    _fields_ = [
        ("normalize", C.c_int32), ("colormap", C.c_int32), ("align_to_world", C.c_int32),
        ("fixed_min", C.c_float), ("fixed_max", C.c_float),
    ]


class FdmGeometry(C.Structure):
    _fields_ = [
        ("length_x", C.c_double), ("length_y", C.c_double), ("resolution", C.c_double),
        ("position_x", C.c_double), ("position_y", C.c_double),
        ("rows", C.c_int32), ("cols", C.c_int32),
        ("start_row", C.c_int32), ("start_col", C.c_int32),
    ]


class FdmTile(C.Structure):
    _fields_ = [
        ("row0", C.c_int32), ("col0", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("own_row0", C.c_int32), ("own_col0", C.c_int32),
        ("own_rows", C.c_int32), ("own_cols", C.c_int32),
    ]


class FdmScanStats(C.Structure):
    _fields_ = [
        ("n_input", C.c_uint32), ("n_after_filter", C.c_uint32),
        ("n_in_map", C.c_uint32), ("n_cells_touched", C.c_uint32),
        ("shift_rows", C.c_int32), ("shift_cols", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FdmRasterStats(C.Structure):  # fdm_raster_stats (include/fdm_engine.h)
    _fields_ = [("n_points_used", C.c_uint64), ("n_cells_written", C.c_uint64)]


class FdmSorStats(C.Structure):  # fdm_sor_stats (include/fdm_engine.h)
    _fields_ = [("n_queries", C.c_uint64), ("n_fallback", C.c_uint64), ("grid_x", C.c_int32), ("grid_y", C.c_int32),
                ("voxel", C.c_float), ("ms", C.c_float * 4)]


class FdmNormalStats(C.Structure):  # fdm_normal_stats (include/fdm_engine.h)
    _fields_ = [("n_queries", C.c_uint64), ("n_fallback", C.c_uint64), ("n_invalid", C.c_uint64),
                ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("voxel", C.c_float), ("ms", C.c_float * 4)]


class FdmAlignSettings(C.Structure):
    """fdm_align_settings == nanopcl::registration::AlignSettings (registration/align.hpp:32-59)."""

    _fields_ = [("max_correspondence_dist", C.c_float), ("max_iterations", C.c_int32), ("translation_eps", C.c_double),
                ("rotation_eps", C.c_double), ("relative_error_eps", C.c_double), ("min_correspondences", C.c_uint64),
                ("robust_kernel", C.c_int32), ("reserved", C.c_int32), ("robust_kernel_width", C.c_double),
                ("covariance_epsilon", C.c_double)]


class FdmRegisterClouds(C.Structure):  # fdm_register_clouds (include/fdm_engine.h)
    _fields_ = [("n_source", C.c_uint64), ("sx", C.c_void_p), ("sy", C.c_void_p), ("sz", C.c_void_p),
                ("s_cov9", C.c_void_p), ("n_target", C.c_uint64), ("tx", C.c_void_p), ("ty", C.c_void_p),
                ("tz", C.c_void_p), ("tnx", C.c_void_p), ("tny", C.c_void_p), ("tnz", C.c_void_p),
                ("t_cov9", C.c_void_p), ("on_device", C.c_int32)]


class FdmRegistrationResult(C.Structure):  # fdm_registration_result
    _fields_ = [("transform", C.c_double * 16), ("fitness", C.c_double), ("rmse", C.c_double),
                ("iterations", C.c_uint64), ("converged", C.c_int32), ("has_covariance", C.c_int32),
                ("covariance", C.c_double * 36)]


class FdmRegisterStats(C.Structure):  # fdm_register_stats
    _fields_ = [("n_source", C.c_uint64), ("n_target", C.c_uint64), ("grid_x", C.c_int32), ("grid_y", C.c_int32),
                ("voxel", C.c_float), ("ring_limit", C.c_int32), ("linearizations", C.c_int32), ("ms", C.c_float * 3)]


class FdmVoxelMapInfo(C.Structure):  # fdm_voxel_map_info
    _fields_ = [("resolution", C.c_float), ("inv_resolution", C.c_float), ("covariance_epsilon", C.c_double),
                ("device", C.c_int32), ("reserved", C.c_int32), ("n_points", C.c_uint64), ("n_skipped", C.c_uint64),
                ("num_voxels", C.c_uint64), ("n_sparse", C.c_uint64), ("table_slots", C.c_uint64),
                ("max_count", C.c_uint32), ("max_probe", C.c_uint32), ("ms", C.c_float * 3), ("reserved2", C.c_float)]


class FdmGroundSegConfig(C.Structure):
    """fdm_ground_seg_config == nanopcl::segmentation::GroundSegConfig (segmentation/ground_seg.hpp:34-40)."""

    _fields_ = [("grid_resolution", C.c_float), ("cell_percentile", C.c_float), ("ground_thickness", C.c_float),
                ("max_ground_height", C.c_float), ("min_points_per_cell", C.c_uint64)]


class FdmRansacConfig(C.Structure):
    """fdm_ransac_config == nanopcl::segmentation::RansacConfig (segmentation/ransac_plane.hpp:104-110)."""

    _fields_ = [("distance_threshold", C.c_float), ("max_iterations", C.c_int32), ("probability", C.c_double),
                ("min_inliers", C.c_uint64), ("refine_model", C.c_int32)]


class FdmRansacResult(C.Structure):  # fdm_ransac_result
    _fields_ = [("coefficients", C.c_float * 4), ("fitness", C.c_double), ("iterations", C.c_int32),
                ("success", C.c_int32), ("n_inliers", C.c_uint64)]


class FdmSegmentStats(C.Structure):  # fdm_segment_stats
    _fields_ = [("n_batches", C.c_uint64), ("n_hypotheses", C.c_uint64), ("n_invalid_samples", C.c_uint64),
                ("batch", C.c_uint32), ("ms", C.c_float * 4)]


class FdmClusterConfig(C.Structure):
    """fdm_cluster_config == nanopcl::segmentation::ClusterConfig (segmentation/euclidean_cluster.hpp:44-48)."""

    _fields_ = [("tolerance", C.c_float), ("min_size", C.c_uint64), ("max_size", C.c_uint64)]


class FdmClusterStats(C.Structure):  # fdm_cluster_stats
    _fields_ = [("n_points", C.c_uint64), ("n_components", C.c_uint64), ("n_kept", C.c_uint64), ("n_rejected", C.c_uint64),
                ("n_clustered", C.c_uint64), ("candidate_pairs", C.c_uint64), ("tests", C.c_uint64),
                ("neighbour_pairs", C.c_uint64), ("unions", C.c_uint64), ("range", C.c_int32), ("key_bits", C.c_uint32),
                ("ms", C.c_float * 6)]


class FdmRorStats(C.Structure):  # fdm_ror_stats
    _fields_ = [("n_points", C.c_uint64), ("candidate_tests", C.c_uint64), ("tests_done", C.c_uint64),
                ("n_kept", C.c_uint64), ("range", C.c_int32), ("key_bits", C.c_uint32), ("ms", C.c_float * 5)]


class FdmCropConfig(C.Structure):  # fdm_crop_config
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


CROP_KIND = {"box": 0, "range": 1, "x": 2, "y": 3, "z": 4, "angle": 5, "finite": 6}
CROP_MODE = {"inside": 0, "outside": 1}
REGISTER_METHOD = {"icp": 0, "plane": 1, "gicp": 2}
ROBUST_KERNEL = {"none": 0, "huber": 1, "tukey": 2, "cauchy": 3}


class FdmDemConfig(C.Structure):
    """fdm_dem_config == fastdem::DEMConfig (io/pcd_convert.hpp:28-42)."""

    _fields_ = [("resolution", C.c_float), ("method", C.c_int32), ("sor_k", C.c_int32), ("sor_std_mul", C.c_float),
                ("height_threshold", C.c_float), ("bin_size", C.c_float), ("inpaint_iterations", C.c_int32)]


class FdmDemStats(C.Structure):  # fdm_dem_stats (include/fdm_engine.h)
    _fields_ = [("n_input", C.c_uint64), ("n_after_sor", C.c_uint64), ("n_after_height", C.c_uint64),
                ("n_sor_fallback", C.c_uint64), ("sor_threshold", C.c_float), ("stage_ms", C.c_float * 7),
                ("raster", FdmRasterStats)]


class FdmCloudView(C.Structure):  # fdm_cloud_view (include/fdm_engine.h)
    _fields_ = [(k, C.c_void_p) for k in ("x", "y", "z", "intensity", "rgb", "nx", "ny", "nz", "cov9")]


class FdmCloudOut(C.Structure):  # fdm_cloud_out (include/fdm_engine.h)
    _fields_ = [(k, C.c_void_p) for k in ("x", "y", "z", "intensity", "rgb", "nx", "ny", "nz", "cov9", "idx")]


class FdmPcdField(C.Structure):  # fdm_pcd_field (include/fdm_engine.h)
    _fields_ = [("name", C.c_char * 64), ("type", C.c_char), ("reserved", C.c_uint8 * 3), ("size", C.c_uint32),
                ("count", C.c_uint32), ("offset", C.c_uint32)]


class FdmPcdHeader(C.Structure):  # fdm_pcd_header (include/fdm_engine.h)
    _fields_ = [("fields", FdmPcdField * 64), ("n_fields", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("point_size", C.c_uint32), ("viewpoint", C.c_double * 7), ("format", C.c_int32),
                ("idx_x", C.c_int32), ("idx_y", C.c_int32), ("idx_z", C.c_int32), ("idx_intensity", C.c_int32),
                ("idx_rgb", C.c_int32), ("idx_nx", C.c_int32), ("idx_ny", C.c_int32), ("idx_nz", C.c_int32),
                ("data_offset", C.c_uint64)]


class FdmRoutePlan(C.Structure):  # fdm_route_plan (include/fdm_engine.h)
    _fields_ = [("world", C.c_int32), ("grid_rows", C.c_int32), ("grid_cols", C.c_int32), ("pad", C.c_int32),
                ("row_edge", C.c_int32 * 17), ("col_edge", C.c_int32 * 17)]


class FdmDeviceScan(C.Structure):  # fdm_device_scan (include/fdm_engine.h)
    _fields_ = [
        ("n", C.c_uint64),
        ("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("intensity", C.c_void_p),
        ("rgb", C.c_void_p), ("sigma_z2", C.c_void_p),
        ("T_base_sensor", C.c_double * 16), ("T_world_base", C.c_double * 16),
    ]


SENSOR_CONSTANT, SENSOR_LIDAR, SENSOR_RGBD = 0, 1, 2
MODE_LOCAL, MODE_GLOBAL = 0, 1
EST_KALMAN, EST_P2 = 0, 1
FDM_OK, FDM_SKIP_EMPTY_CLOUD, FDM_SKIP_ALL_FILTERED, FDM_SKIP_NO_CELL, FDM_SKIP_BUFFER_TOO_SMALL = 0, 1, 2, 3, 4
RASTER_METHOD = {"max": 0, "min": 1, "mean": 2, "minmax": 3}        # fastdem::RasterMethod
FDM_ERR_INVALID, FDM_ERR_HIP, FDM_ERR_NO_LAYER, FDM_ERR_NO_DEVICE = -1, -2, -3, -4
NORMALIZE = {"min_max": 0, "percentile_1_99": 1, "fixed_range": 2}   # PngExportConfig::Normalize
VOXEL_MODE = {"centroid": 0, "nearest": 1, "any": 2, "center": 3}   # nanopcl::filters::VoxelMode
PCD_ASCII, PCD_BINARY = 0, 1                                         # fdm_pcd_header.format
COLORMAP = {"grayscale": 0, "viridis": 1, "jet": 2}                  # PngExportConfig::Colormap

_P = C.c_void_p
_F = C.POINTER(C.c_float)
_U = C.POINTER(C.c_uint32)
_D = C.POINTER(C.c_double)

# name -> (restype, argtypes): every symbol include/fdm_engine.h declares
PROTOTYPES = {
    "fdm_default_config": (None, [C.POINTER(FdmConfig)]),
    "fdm_last_error": (C.c_char_p, []),
    "fdm_engine_create": (C.c_int, [C.POINTER(FdmGeometry), C.POINTER(FdmConfig),
                                    C.POINTER(FdmTile), C.c_int, C.POINTER(_P)]),
    "fdm_engine_create_map": (C.c_int, [C.POINTER(FdmGeometry), C.POINTER(FdmTile), C.c_int,
                                        C.POINTER(_P)]),
    "fdm_engine_destroy": (None, [_P]),
    "fdm_engine_set_config": (C.c_int, [_P, C.POINTER(FdmConfig)]),
    "fdm_engine_set_stream": (C.c_int, [_P, _P]),
    "fdm_engine_integrate": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, _D, _D,
                                       C.POINTER(FdmScanStats)]),
    "fdm_engine_integrate_points4": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _D, _D, C.POINTER(FdmScanStats)]),
    "fdm_engine_integrate_device": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, _D, _D]),
    "fdm_engine_integrate_device_batch": (C.c_int, [_P, C.c_uint32, _P]),
    "fdm_engine_integrate_device_batch_timed": (C.c_int, [_P, C.c_uint32, _P]),
    "fdm_engine_integrate_host_batch": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "fdm_engine_integrate_async": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_double),
                                             C.POINTER(C.c_double)]),
    "fdm_engine_route_scan": (C.c_int, [_P, C.POINTER(FdmRoutePlan), C.c_uint64, _P, _P, _P, _P, _D, _D, _P, _P]),
    "fdm_engine_integrate_points4_device": (C.c_int, [_P, C.c_uint64, _P, C.c_int, C.c_int, _D, _D]),
    "fdm_engine_route_scan_soa": (C.c_int, [_P, C.POINTER(FdmRoutePlan), C.c_uint64, _P, _P, _P, _P, _D, _D, _P, _P]),
    "fdm_engine_integrate_soa4_device": (C.c_int, [_P, C.c_uint64, _P, C.c_int, C.c_int, _D, _D]),
    "fdm_engine_update": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, C.c_double,
                                    C.c_double, C.POINTER(FdmScanStats)]),
    "fdm_engine_update_device": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, C.c_double,
                                           C.c_double]),
    "fdm_host_alloc": (_P, [C.c_uint64]),
    "fdm_host_free": (None, [_P]),
    "fdm_host_trim": (None, []),
    "fdm_host_is_pinned": (C.c_int, [_P]),
    "fdm_engine_flush": (C.c_int, [_P]),
    "fdm_engine_stream": (_P, [_P]),
    "fdm_engine_last_pipeline": (C.c_int, [_P]),
    "fdm_engine_last_batch": (C.c_int, [_P]),
    "fdm_engine_timer_start": (C.c_int, [_P]),
    "fdm_engine_timer_stop": (C.c_int, [_P]),
    "fdm_engine_timer_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "fdm_engine_debug_batch_dirty": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "fdm_engine_debug_batch_launches": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "fdm_engine_debug_last_post_kernel": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "fdm_engine_debug_timeline": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fdm_engine_record_event": (C.c_int, [_P, _P]),
    "fdm_engine_wait_event": (C.c_int, [_P, _P]),
    "fdm_engine_sync": (C.c_int, [_P]),
    "fdm_engine_last_stats": (C.c_int, [_P, C.POINTER(FdmScanStats)]),
    "fdm_engine_move": (C.c_int, [_P, C.c_double, C.c_double]),
    "fdm_engine_get_geometry": (C.c_int, [_P, C.POINTER(FdmGeometry)]),
    "fdm_engine_set_position": (C.c_int, [_P, C.c_double, C.c_double]),
    "fdm_engine_set_start_index": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "fdm_engine_num_layers": (C.c_int, [_P]),
    "fdm_engine_layer_name": (C.c_char_p, [_P, C.c_int]),
    "fdm_engine_layer_exists": (C.c_int, [_P, C.c_char_p]),
    "fdm_engine_layer_add": (C.c_int, [_P, C.c_char_p, C.c_float]),
    "fdm_engine_layer_download": (C.c_int, [_P, C.c_char_p, _P, C.c_int32, C.c_int32]),
    "fdm_engine_layer_upload": (C.c_int, [_P, C.c_char_p, _P, C.c_int32, C.c_int32]),
    "fdm_engine_layer_device_ptr": (_P, [_P, C.c_char_p]),
    "fdm_engine_clear": (C.c_int, [_P, C.c_char_p]),
    "fdm_engine_layer_copy": (C.c_int, [_P, _P, C.c_char_p]),
    "fdm_engine_region_pack": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(C.c_char_p), C.c_int, _P]),
    "fdm_engine_region_unpack": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.POINTER(C.c_char_p), C.c_int, _P]),
    "fdm_engine_regions_pack": (C.c_int, [_P, C.c_int32, _P, C.POINTER(C.c_char_p), C.c_int, _P]),
    "fdm_engine_regions_unpack": (C.c_int, [_P, C.c_int32, _P, C.POINTER(C.c_char_p), C.c_int, _P]),
    "fdm_engine_capture": (C.c_int, [_P, C.c_int, C.c_int]),
    "fdm_engine_last_preprocessed": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "fdm_engine_last_preprocessed_cov": (C.c_int, [_P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "fdm_engine_last_rasterized": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "fdm_engine_apply_raycasting": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _F, C.POINTER(FdmRaycastConfig)]),
    "fdm_engine_apply_raycasting_device": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _F,
                                                     C.POINTER(FdmRaycastConfig)]),
    "fdm_engine_voxel_any": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.c_float, _P, C.POINTER(C.c_uint64)]),
    "fdm_engine_last_ray_ms": (C.c_int, [_P, _F]),
    "fdm_engine_apply_inpainting": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "fdm_engine_apply_spatial_smoothing": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int]),
    "fdm_engine_apply_uncertainty_fusion": (C.c_int, [_P, C.POINTER(FdmFusionConfig)]),
    "fdm_engine_apply_feature_extraction": (C.c_int, [_P, C.c_float, C.c_int, C.c_float, C.c_float]),
    "fdm_engine_ingest_cloud2": (C.c_int, [_P, _P, C.c_int, C.c_uint64, C.POINTER(FdmCloud2Layout),
                                           C.POINTER(C.c_uint64)]),
    "fdm_engine_ingested": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                                      C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "fdm_engine_integrate_cloud2": (C.c_int, [_P, _P, C.c_int, C.c_uint64, C.POINTER(FdmCloud2Layout),
                                              C.POINTER(C.c_double), C.POINTER(C.c_double),
                                              C.POINTER(FdmScanStats)]),
    "fdm_engine_pack_cloud": (C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                        C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                        C.c_char_p, C.c_uint64]),
    "fdm_engine_pack_cloud_device": (C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.POINTER(_P), C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint32)]),
    "fdm_engine_from_point_cloud": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, C.c_int, C.POINTER(FdmRasterStats)]),
    "fdm_engine_from_point_cloud_device": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, C.c_int,
                                                     C.POINTER(FdmRasterStats)]),
    "fdm_engine_create_from_point_cloud": (C.c_int, [C.c_uint64, _P, _P, _P, _P, _P, C.c_int, C.c_float, C.c_int, C.c_int,
                                                     C.POINTER(_P), C.POINTER(FdmRasterStats)]),
    "fdm_engine_to_point_cloud": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "fdm_engine_to_point_cloud_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                                                   C.POINTER(_P), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_int32)]),
    "fdm_engine_last_raster_ms": (C.c_int, [_P, _F]),
    "fdm_statistical_outlier_removal": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_int, _P, _P,
                                                  _F, C.POINTER(C.c_uint64)]),
    "fdm_sor_last_stats": (C.c_int, [C.POINTER(FdmSorStats)]),
    "fdm_engine_remove_floating_points": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.c_int, C.c_float, C.c_float, _P,
                                                    C.POINTER(C.c_uint64)]),
    "fdm_cloud_voxel_grid": (C.c_int, [C.c_uint64, C.POINTER(FdmCloudView), C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(FdmCloudOut), C.POINTER(C.c_uint64)]),
    "fdm_cloud_grid_max_z": (C.c_int, [C.c_uint64, C.POINTER(FdmCloudView), C.c_int, C.c_float, C.c_int, C.c_int,
                                       C.POINTER(FdmCloudOut), C.POINTER(C.c_uint64)]),
    "fdm_cloud_estimate_normals": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P,
                                             C.POINTER(C.c_uint64)]),
    "fdm_normals_last_stats": (C.c_int, [C.POINTER(FdmNormalStats)]),
    "fdm_default_align_settings": (None, [C.POINTER(FdmAlignSettings)]),
    "fdm_cloud_register": (C.c_int, [C.c_int, C.POINTER(FdmRegisterClouds), _P, C.POINTER(FdmAlignSettings), C.c_int,
                                     C.POINTER(FdmRegistrationResult)]),
    "fdm_cloud_register_linearize": (C.c_int, [C.c_int, C.POINTER(FdmRegisterClouds), _P, C.POINTER(FdmAlignSettings),
                                               C.c_int, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), _P]),
    "fdm_register_last_stats": (C.c_int, [C.POINTER(FdmRegisterStats)]),
    "fdm_voxel_map_create": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, C.c_float, C.c_double, C.c_int, C.POINTER(_P)]),
    "fdm_voxel_map_destroy": (None, [_P]),
    "fdm_voxel_map_get_info": (C.c_int, [_P, C.POINTER(FdmVoxelMapInfo)]),
    "fdm_voxel_map_records": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "fdm_cloud_register_vgicp": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, C.c_int, _P, C.POINTER(FdmAlignSettings),
                                           C.POINTER(FdmRegistrationResult)]),
    "fdm_cloud_register_vgicp_linearize": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, C.c_int, _P,
                                                     C.POINTER(FdmAlignSettings), _P, _P, C.POINTER(C.c_double),
                                                     C.POINTER(C.c_uint64), _P]),
    "fdm_cloud_segment_ground": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, C.POINTER(FdmGroundSegConfig), C.c_int, _P, _P,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fdm_cloud_segment_plane": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, _P, C.c_uint64, C.POINTER(FdmRansacConfig),
                                          C.c_int, _P, C.POINTER(FdmRansacResult)]),
    "fdm_cloud_segment_planes": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, C.POINTER(FdmRansacConfig), C.c_uint64,
                                           C.c_double, C.c_int, _P, C.POINTER(FdmRansacResult), C.POINTER(C.c_uint64)]),
    "fdm_segment_last_stats": (C.c_int, [C.POINTER(FdmSegmentStats)]),
    "fdm_segment_debug_batch": (C.c_int, [C.c_int]),
    "fdm_cloud_cluster": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, _P, C.c_uint64, C.POINTER(FdmClusterConfig), C.c_int,
                                    _P, _P, _P, C.POINTER(C.c_uint64)]),
    "fdm_cluster_last_stats": (C.c_int, [C.POINTER(FdmClusterStats)]),
    "fdm_cloud_radius_outlier_removal": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, C.c_float, C.c_uint64, C.c_int, _P, _P,
                                                   C.POINTER(C.c_uint64)]),
    "fdm_ror_last_stats": (C.c_int, [C.POINTER(FdmRorStats)]),
    "fdm_cloud_crop": (C.c_int, [C.c_uint64, _P, _P, _P, C.c_int, C.POINTER(FdmCropConfig), C.c_int, _P,
                                 C.POINTER(C.c_uint64)]),
    "fdm_cloud_debug_profile": (C.c_int, [C.c_int]),
    "fdm_cloud_debug_last_ms": (C.c_int, [_F]),
    "fdm_default_dem_config": (None, [C.POINTER(FdmDemConfig)]),
    "fdm_engine_build_dem": (C.c_int, [C.c_uint64, _P, _P, _P, _P, _P, C.c_int, C.POINTER(FdmDemConfig), C.c_int,
                                       C.POINTER(_P), C.POINTER(FdmDemStats)]),
    "fdm_pcd_parse_header": (C.c_int, [_P, C.c_uint64, C.POINTER(FdmPcdHeader)]),
    "fdm_pcd_write_header": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, _D, C.c_int, _P, C.c_uint64,
                                       C.POINTER(C.c_uint64)]),
    "fdm_pcd_decode": (C.c_int, [C.POINTER(FdmPcdHeader), _P, C.c_uint64, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int,
                                 C.c_int]),
    "fdm_pcd_encode": (C.c_int, [C.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                 C.c_uint64, C.POINTER(C.c_uint64)]),
    "fdm_pcd_build_dem": (C.c_int, [C.POINTER(FdmPcdHeader), _P, C.c_uint64, C.c_int, C.POINTER(FdmDemConfig), C.c_int,
                                    C.POINTER(_P), C.POINTER(FdmDemStats)]),
    "fdm_engine_to_pcd": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "fdm_pcd_debug_profile": (C.c_int, [C.c_int]),
    "fdm_pcd_debug_last_kernel_ms": (C.c_int, [_F]),
    "fdm_default_image_config": (None, [C.POINTER(FdmImageConfig)]),
    "fdm_engine_render_layer": (C.c_int, [_P, C.c_char_p, C.POINTER(FdmImageConfig), _P, C.c_uint64,
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F]),
    "fdm_engine_render_layer_device": (C.c_int, [_P, C.c_char_p, C.POINTER(FdmImageConfig), C.POINTER(_P),
                                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F]),
    "fdm_engine_enable_cell_ids": (C.c_int, [_P, C.c_int]),
    "fdm_engine_last_cell_ids": (C.c_int, [_P, _P, C.c_uint64]),
    "fdm_engine_enable_profile": (C.c_int, [_P, C.c_int]),
    "fdm_engine_last_kernel_ms": (C.c_int, [_P, _F]),
    "fdm_engine_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
}

_lib = None


def load():
    """dlopen libfdm_engine.so (after torch, so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  fastdem_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 first; ours resolves to the same soname)
    except Exception:  # pragma: no cover - torch is plumbing, the library works without it
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here == header/library drift
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def default_config():
    cfg = FdmConfig()
    load().fdm_default_config(C.byref(cfg))
    return cfg


def default_dem_config():
    cfg = FdmDemConfig()
    load().fdm_default_dem_config(C.byref(cfg))
    return cfg


def default_image_config():
    cfg = FdmImageConfig()
    load().fdm_default_image_config(C.byref(cfg))
    return cfg


def stats_dict(st):
    """A statistics struct as a dict: integer fields as int, floating-point fields as float, arrays as tuples of float;
    `reserved*` fields are left out."""
    out = {}
    for name, _ in st._fields_:
        if not name.startswith("reserved"):
            v = getattr(st, name)
            out[name] = v if isinstance(v, (int, float)) else tuple(float(e) for e in v)
    return out
