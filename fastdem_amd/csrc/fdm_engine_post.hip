// fdm_engine_post.hip — the stages behind the hot path: stencil post-processing (fdm_post.hpp),
// map egress (fdm_egress.hpp), layer images (fdm_render.hpp), PointCloud2 ingest (fdm_ingest.hpp),
// static point clouds to and from the map (fdm_raster.hpp), buildDEM and its filter stages (fdm_knn.hpp, fdm_dem.hpp),
// normal and covariance estimation (fdm_normals.hpp), cloud registration (fdm_register.hpp, fdm_vgicp.hpp), cloud segmentation
// (fdm_segment.hpp, fdm_segment_host.hpp), Euclidean clustering (fdm_cluster.hpp, fdm_cluster_host.hpp), the cloud filters (fdm_filter.hpp, fdm_filter_host.hpp), PCD files (fdm_pcd.hpp, fdm_pcd_host.hpp).  At its head fdm_engine_cloud.inl: what the host files of the cloud and
// file stages share (scoped scratch, the cloud staging, the argument checks, the map over a cloud, the pack counters).
// One of the library's five translation units (fdm_engine_host.hpp).
#include "fdm_engine_host.hpp"
#include "fdm_filter.hpp"

#include "fdm_engine_cloud.inl"
#include "fdm_engine_post.inl"
#include "fdm_engine_io.inl"
#include "fdm_engine_render.inl"
#include "fdm_engine_raster.inl"
#include "fdm_engine_dem.inl"
#include "fdm_engine_normals.inl"
#include "fdm_engine_register.inl"
#include "fdm_engine_segment.inl"
#include "fdm_engine_vgicp.inl"
#include "fdm_engine_cluster.inl"
#include "fdm_engine_filter.inl"
#include "fdm_engine_pcd.inl"
