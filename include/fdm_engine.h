/* fdm_engine.h — C ABI of the MI355X elevation-map update engine (libfdm_engine.so).
 *
 * This is the drop-in boundary for ONE path of Ikhyeon-Cho/FastDEM:
 *   fastdem::FastDEM::integrate(cloud, T_base_sensor, T_world_base)
 * The reference has no FFI; its boundary is the C++ class surface
 * (fastdem/include/fastdem/fastdem.hpp:54-158).  A maintainer swaps the body of
 * FastDEM::integrateImpl (fastdem/src/fastdem.cpp:133-162) for the calls below —
 * INTEGRATION.md shows the binding.  Every entry point cites what it replaces.
 *
 * Conventions
 *   - plain pointers and sizes; no C++/torch types; no exceptions cross the boundary
 *   - int status: 0 ok, >0 "skipped" (the reference's `return false` cases), <0 error
 *   - transforms are column-major double[16] == Eigen::Isometry3d::matrix().data()
 *   - layers are float32, column-major rows x cols == Eigen::MatrixXf storage
 *     (fastdem/include/fastdem/bridge/ros/impl.hpp:117-119)
 *   - one engine = one device + one HIP stream; not thread-safe, caller serialises
 *     (same contract as fastdem.hpp:48-53)
 *   - host pointers are borrowed for the duration of the call only (pinned arrays handed to the
 *     enqueue-only fdm_engine_integrate_async: until the work that call enqueued has run); device
 *     pointers passed to the *_device entry points follow the ordinary stream contract — free to
 *     reuse once the work the call enqueued has run (fdm_engine_record_event / fdm_engine_sync);
 *     a held-back map update never reads them (see fdm_engine_integrate_device)
 */
#ifndef FDM_ENGINE_H
#define FDM_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fdm_engine fdm_engine;

/* Mirrors fastdem::Config for this path, field for field
 * (config/fastdem.hpp:23-38, config/sensor_model.hpp:10-37, config/mapping.hpp:10-48).
 * The last six fields are config::Raycasting (config/postprocess.hpp:16-23). */
typedef struct fdm_config {
  float z_min, z_max, range_min, range_max;     /* config::PointFilter */
  int32_t sensor_type;                          /* SensorType: 0 Constant, 1 LiDAR, 2 RGBD */
  float lidar_range_noise, lidar_angular_noise;
  float rgbd_normal_a, rgbd_normal_b, rgbd_normal_c, rgbd_lateral_factor;
  float constant_uncertainty;
  int32_t mode;                                 /* MappingMode: 0 LOCAL, 1 GLOBAL */
  int32_t estimation_type;                      /* EstimationType: 0 Kalman, 1 P2Quantile */
  float kalman_min_variance, kalman_max_variance, kalman_process_noise;
  float p2_dn[5];
  int32_t p2_elevation_marker;
  float p2_max_sample_count;
  int32_t raycast_enabled;                      /* config::Raycasting::enabled (default 0) */
  float rc_height_conflict_threshold, rc_log_odds_observed, rc_log_odds_ghost, rc_log_odds_max,
      rc_clear_threshold;
} fdm_config;

/* config::Raycasting on its own (config/postprocess.hpp:16-23), for applyRaycasting called directly. */
typedef struct fdm_raycast_config {
  int32_t enabled;
  float height_conflict_threshold, log_odds_observed, log_odds_ghost, log_odds_max, clear_threshold;
} fdm_raycast_config;

/* nanogrid::GridMap geometry (length, resolution, position, circular-buffer start).
 * rows/cols are outputs of create (size = round(length / resolution)). */
typedef struct fdm_geometry {
  double length_x, length_y, resolution, position_x, position_y;
  int32_t rows, cols, start_row, start_col;
} fdm_geometry;

/* Multi-GPU spatial tiling, GLOBAL mode only.  This engine STORES the
 * window [row0,row0+rows) x [col0,col0+cols) of the global buffer (owned cells plus a
 * read-only halo ring) and UPDATES only the owned window [own_row0,own_row0+own_rows) x
 * [own_col0,own_col0+own_cols); points landing elsewhere are ignored by this engine.
 * Cell indices are always computed against the GLOBAL geometry, so they are bit-identical
 * to the single-GPU map. */
typedef struct fdm_tile {
  int32_t row0, col0, rows, cols;
  int32_t own_row0, own_col0, own_rows, own_cols;
} fdm_tile;

typedef struct fdm_scan_stats {
  uint32_t n_input;         /* points handed in */
  uint32_t n_after_filter;  /* survived cropRange + cropZ (fastdem.cpp:175-176) */
  uint32_t n_in_map;        /* getIndex succeeded (elevation_mapping.cpp:55) */
  uint32_t n_cells_touched; /* |CellObservations| */
  int32_t shift_rows, shift_cols; /* index shift of the LOCAL-mode move applied */
} fdm_scan_stats;

enum {
  FDM_OK = 0,
  FDM_SKIP_EMPTY_CLOUD = 1,   /* fastdem.cpp:125-128 -> false */
  FDM_SKIP_ALL_FILTERED = 2,  /* fastdem.cpp:138     -> false */
  FDM_SKIP_NO_CELL = 3,       /* pcd_convert.cpp:103: no point of the cloud landed in a cell */
  FDM_SKIP_BUFFER_TOO_SMALL = 4, /* fdm_engine_to_point_cloud: the cloud has more points than the arrays hold */
  FDM_ERR_INVALID = -1,
  FDM_ERR_HIP = -2,
  FDM_ERR_NO_LAYER = -3,
  FDM_ERR_NO_DEVICE = -4
};

void fdm_default_config(fdm_config* cfg);      /* Config{} defaults */
const char* fdm_last_error(void);              /* text of the last <0 status on this thread */

/* ElevationMap(width,height,resolution,frame) + FastDEM(map,cfg) construction
 * (elevation_map.hpp:101-116, fastdem.cpp:19-22, elevation_mapping.cpp:11-39):
 * allocates the layers in HBM with the reference's initial constants.
 * g->length_*, resolution, position_* are read; tile may be NULL (whole map). */
int fdm_engine_create(const fdm_geometry* g, const fdm_config* cfg, const fdm_tile* tile,
                      int device, fdm_engine** out);
/* ElevationMap(width,height,resolution,frame) ALONE (elevation_map.hpp:101-116): the three
 * default layers, no estimator layers yet.  fdm_engine_set_config() then plays the role of
 * constructing FastDEM / ElevationMapping on that map (ensureLayers + obstacle layer). */
int fdm_engine_create_map(const fdm_geometry* g, const fdm_tile* tile, int device, fdm_engine** out);
void fdm_engine_destroy(fdm_engine* e);

/* FastDEM fluent setters (fastdem.cpp:28-62): filters/sensor params take effect on
 * the next scan; a new estimator type adds its layers, the old ones persist. */
int fdm_engine_set_config(fdm_engine* e, const fdm_config* cfg);

/* Run on the caller's HIP stream (hipStream_t as void*; NULL = engine's own stream). */
int fdm_engine_set_stream(fdm_engine* e, void* hip_stream);

/* FastDEM::integrate(const PointCloud&, T_base_sensor, T_world_base) — fastdem.cpp:122-162.
 * SoA host arrays (x,y,z required; intensity / rgb = 0x00RRGGBB / sigma_z2 nullable).
 * sigma_z2, when given, replaces the built-in sensor model: it is the (2,2) element of
 * R*Sigma*R^T per point, for user SensorModel subclasses (fastdem.hpp:79-80).
 * Synchronous: returns after the map update; status as above. */
int fdm_engine_integrate(fdm_engine* e, uint64_t n, const float* x, const float* y,
                         const float* z, const float* intensity, const uint32_t* rgb,
                         const float* sigma_z2, const double T_base_sensor[16],
                         const double T_world_base[16], fdm_scan_stats* out);

/* Same, inputs already resident in HBM; enqueue-only (no host sync).  The skip
 * decisions of fastdem.cpp:125-138 are taken on the device; read them back with
 * fdm_engine_last_stats().
 * The map update of the scan is HELD BACK and leaves in the same launch as the next scan's bin kernel
 * (one launch per scan instead of two); every other entry point — fdm_engine_sync() included — first
 * launches a held-back update, so the map is always current when it is read through this API.
 * A caller that reads layers through raw device pointers on its own stream orders itself behind
 * fdm_engine_record_event() (which launches the held-back update first).
 * Input arrays follow the ordinary stream contract: they may be reused as soon as the work this call
 * enqueued has run (an event from fdm_engine_record_event, or fdm_engine_sync) — the held-back update
 * never reads them (the bin kernel leaves what it needs in engine-owned memory).  Producers on another
 * stream hand the arrays over with fdm_engine_wait_event().
 * fdm_engine_set_option(e, "overlap", 0) turns the hold-back off. */
int fdm_engine_integrate_device(fdm_engine* e, uint64_t n, const float* d_x, const float* d_y,
                                const float* d_z, const float* d_intensity, const uint32_t* d_rgb,
                                const float* d_sigma_z2, const double T_base_sensor[16],
                                const double T_world_base[16]);

/* A batch of device-resident scans in ONE call (a bag replay, a driver that queues ahead): the map it leaves is
 * exactly what `count` consecutive fdm_engine_integrate_device calls leave (every layer bit for bit), without the
 * per-call crossing of the language boundary — and, because the engine sees the scans up front, without one launch
 * per scan: runs of small plain scans of one sensor (same T_base_sensor, same optional channels, no captures / cell
 * ids, a map of at most 2^18 cells) are binned sixteen to a launch and applied cell by cell in scan order by the
 * same launch's update half (fastdem_amd/csrc/fdm_multi.hpp; configs[1]: 1.05 us instead of 4-6 us per scan).  With
 * raycast_enabled (fastdem.cpp:152-159) the stage of every scan rides in the batch as well — voxel filter, ray walks,
 * ghost resolution, each scan's behind that scan's map update (fdm_rbatch.hpp; scans of <= 64 K points on an untiled
 * engine; 9.3 us instead of 60 us per VLP-16 scan).  Scans that do not qualify take the single-scan path in place.
 * Options "batch" 0/1, "batch_max" 0 (automatic: 32 with the quantile estimator or with raycasting on, 16 with Kalman alone) or 2..32, "batch_ray" 0/1. */
typedef struct fdm_device_scan {
  uint64_t n;
  const float *x, *y, *z, *intensity; /* device pointers; intensity nullable */
  const uint32_t* rgb;                /* nullable */
  const float* sigma_z2;              /* nullable */
  double T_base_sensor[16];           /* column-major */
  double T_world_base[16];
} fdm_device_scan;
int fdm_engine_integrate_device_batch(fdm_engine* e, uint32_t count, const fdm_device_scan* scans);
/* Returns FDM_OK or the first error (< 0); an empty cloud in the batch is skipped and the batch goes on. */
/* The same for HOST clouds (the pointers of `host_scans` are host pointers): N consecutive FastDEM::integrate calls —
 * a bag replay, a driver that hands over the scans of the last 100 ms — in batch launches.  Pinned channels
 * (fdm_host_alloc: every nanopcl::PointCloud of the C++ mirror) are read in place over PCIe, once; pageable ones are
 * staged.  out_last != NULL: waits and returns the LAST scan's status and statistics like fdm_engine_integrate;
 * NULL: enqueue-only — pinned clouds must then stay untouched until fdm_engine_sync(). */
int fdm_engine_integrate_host_batch(fdm_engine* e, uint32_t count, const fdm_device_scan* host_scans,
                                    fdm_scan_stats* out_last);

/* FastDEM::integrate(cloud, T_base_sensor, T_world_base) on the reference's own point layout — replaces
 * fastdem/src/fastdem.cpp:122-190 for a caller that holds a nanopcl::PointCloud: `xyz1` = cloud.points().data(), n
 * contiguous 16-byte {x, y, z, 1} records (nanopcl/core/point_cloud.hpp:126-134, core/types.hpp:19-22), HOST memory,
 * 16-byte aligned.  Pinned memory (fdm_host_alloc / hipHostMalloc) is read in place, once, over PCIe; pageable memory
 * is copied first.  intensity / rgb / sigma_z2: the optional channels, separate host arrays of n entries (nullable), as
 * in fdm_engine_integrate.  Synchronous; status and statistics as fdm_engine_integrate. */
int fdm_engine_integrate_points4(fdm_engine* e, uint64_t n, const float* xyz1, const float* intensity,
                                 const uint32_t* rgb, const float* sigma_z2, const double T_base_sensor[16],
                                 const double T_world_base[16], fdm_scan_stats* out);

/* Same, HOST arrays, enqueue-only; nothing waits.  For a stream of scans from host memory (bag replay,
 * a ROS callback).
 *   PINNED arrays (fdm_host_alloc / hipHostMalloc / hipHostRegister): no copy is queued — the bin kernel
 *     reads the arrays in place over PCIe (once) and leaves a copy in an HBM staging block for the
 *     update kernel; one launch per scan.  Keep a scan's arrays untouched until its launch has run
 *     (fdm_engine_sync(), or an event recorded on fdm_engine_stream()).
 *   pageable arrays: copied into a rotating staging block with hipMemcpyAsync (which the runtime
 *     stages, i.e. the call blocks for the copy), scan enqueued behind the copies.
 * The synchronous host entry points (fdm_engine_integrate, fdm_engine_update) make the same choice.
 * fdm_engine_set_option(e, "zero_copy", max_points) bounds the in-place path (0 = always copy). */
int fdm_engine_integrate_async(fdm_engine* e, uint64_t n, const float* x, const float* y,
                               const float* z, const float* intensity, const uint32_t* rgb,
                               const float* sigma_z2, const double T_base_sensor[16],
                               const double T_world_base[16]);

/* ElevationMapping::update(cloud, robot_position) — elevation_mapping.cpp:110-125 —
 * for a cloud already in the map frame (tests/test_dual_layer.cpp:71).  z_var NULL
 * == cloud without covariance channel (pt_z_var = 0, elevation_mapping.cpp:57-60). */
int fdm_engine_update(fdm_engine* e, uint64_t n, const float* x, const float* y, const float* z,
                      const float* z_var, const float* intensity, const uint32_t* rgb,
                      double robot_x, double robot_y, fdm_scan_stats* out);
int fdm_engine_update_device(fdm_engine* e, uint64_t n, const float* d_x, const float* d_y,
                             const float* d_z, const float* d_z_var, const float* d_intensity,
                             const uint32_t* d_rgb, double robot_x, double robot_y);

/* Launch a held-back map update now, without waiting for it (see fdm_engine_integrate_device). */
int fdm_engine_flush(fdm_engine* e);
/* The HIP stream (hipStream_t) the engine launches on: for callers that bracket engine work with
 * their own HIP events or order their own kernels after it. */
void* fdm_engine_stream(fdm_engine* e);
/* Which pipeline the last scan took: 0 = per-cell scratch (k_bin / k_update), 1 = per-tile record pools
 * (k_tbin / k_tupdate: maps of >= 240 tiles of 32 x 32 cells, scans of >= 2 K points), -1 = no scan yet.  Diagnostic. */
int fdm_engine_last_pipeline(fdm_engine* e);
/* Scans of the batch launch the last scan left in (fdm_engine_integrate_device_batch groups up to 16 small scans
 * per launch, see below), 0 when it took the single-scan path.  Diagnostic. */
int fdm_engine_last_batch(fdm_engine* e);
/* Device-side stopwatch on the engine's stream (two engine-owned HIP events): _start marks "everything enqueued so
 * far" (a held-back update is launched first), _stop launches the last scan's held-back update and marks its end,
 * _ms waits for the stop mark and returns the time between the two.  For callers without HIP of their own that
 * want the GPU's view of a run of enqueue-only calls (bench.py's `device_value`). */
int fdm_engine_timer_start(fdm_engine* e);
int fdm_engine_timer_stop(fdm_engine* e);
int fdm_engine_timer_ms(fdm_engine* e, float* ms);
/* Order a consumer behind the engine: launches a held-back update, then records `hip_event`
 * (hipEvent_t) on the engine's stream — everything enqueued so far, the map update of the last scan
 * included, is complete when the event fires (the reference's callers hold a shared_mutex around
 * integrate() for this, fastdem.hpp:48-53). */
int fdm_engine_record_event(fdm_engine* e, void* hip_event);
/* Order the engine behind a producer: work enqueued after this call waits for `hip_event`
 * (hipStreamWaitEvent), e.g. the kernel or copy that fills the next scan's device arrays. */
int fdm_engine_wait_event(fdm_engine* e, void* hip_event);
int fdm_engine_sync(fdm_engine* e);
/* Waits for the stream, returns the status (0/1/2) and stats of the last enqueued scan. */
int fdm_engine_last_stats(fdm_engine* e, fdm_scan_stats* out);

/* nanogrid::GridMap::move(Position) (elevation_mapping.cpp:113): rolling-window shift. */
int fdm_engine_move(fdm_engine* e, double x, double y);
int fdm_engine_get_geometry(fdm_engine* e, fdm_geometry* out);       /* getPosition/getStartIndex/... */
int fdm_engine_set_position(fdm_engine* e, double x, double y);      /* GridMap::setPosition */
int fdm_engine_set_start_index(fdm_engine* e, int32_t row, int32_t col);

/* GridMap::getLayers / exists / add / get / clear / clearAll (FastDEM::reset = clear(NULL)).
 * A map holds at most 128 layers, the estimator's own among them; adding one more is FDM_ERR_INVALID
 * (the reference has no such bound). */
int fdm_engine_num_layers(fdm_engine* e);
const char* fdm_engine_layer_name(fdm_engine* e, int i);
int fdm_engine_layer_exists(fdm_engine* e, const char* name);
int fdm_engine_layer_add(fdm_engine* e, const char* name, float value);
int fdm_engine_layer_download(fdm_engine* e, const char* name, float* host, int32_t rows, int32_t cols);
int fdm_engine_layer_upload(fdm_engine* e, const char* name, const float* host, int32_t rows, int32_t cols);
float* fdm_engine_layer_device_ptr(fdm_engine* e, const char* name); /* NULL if absent or if the layer is
                                                                      a field of the packed cell records */
int fdm_engine_clear(fdm_engine* e, const char* name /* NULL = clearAll */);
/* Copy of a map, layer by layer, device to device (ElevationMap's copy constructor / snapshot(), elevation_map.hpp:95-99;
 * the ROS node's copy under a shared lock, ros1/src/fastdem_ros_node.cpp:192-199): layer `name` of `src` into `dst`
 * (created there if missing).  Both engines on one device with the same stored window. */
int fdm_engine_layer_copy(fdm_engine* dst, fdm_engine* src, const char* name);

/* Halo exchange support for spatial tiling: pack the rectangle [r0,r0+nr) x [c0,c0+nc)
 * (storage-local indices) of `n_layers` named layers into a contiguous device buffer
 * (layer-major, each rectangle column-major), or write such a buffer back.  The RCCL
 * send/recv between neighbouring ranks is done by the caller (fastdem_amd/tiling.py). */
int fdm_engine_region_pack(fdm_engine* e, int32_t r0, int32_t c0, int32_t nr, int32_t nc,
                           const char* const* names, int n_layers, float* d_buf);
int fdm_engine_region_unpack(fdm_engine* e, int32_t r0, int32_t c0, int32_t nr, int32_t nc,
                             const char* const* names, int n_layers, const float* d_buf);
/* The same for several rectangles at once — ONE launch for all the strips and layers of a halo exchange (up to 8
 * rectangles x 24 layers per launch): rectangle q's block starts at float `offset` of d_buf and is laid out as
 * above (layer-major over the n_layers, column-major inside). */
typedef struct fdm_region {
  int32_t r0, c0, nr, nc;
  uint64_t offset;
} fdm_region;
int fdm_engine_regions_pack(fdm_engine* e, int32_t n_rects, const fdm_region* rects, const char* const* names,
                            int n_layers, float* d_buf);
int fdm_engine_regions_unpack(fdm_engine* e, int32_t n_rects, const fdm_region* rects, const char* const* names,
                              int n_layers, const float* d_buf);

/* ---- Scan routing for a spatially tiled global map (fastdem_amd/tiling.py, include/fdm_halo.h) ----
 * One logical scan = the concatenation, in rank order, of per-rank slices.  fdm_engine_route_scan runs a slice through
 * T_base_sensor, cropRange, cropZ, T_world_base and getIndex against the GLOBAL geometry — the operations the owner's
 * bin kernel repeats — and partitions the slice's RAW points by the rank that owns the cell they fall into, order
 * preserved: d_send receives {x, y, z, intensity} records (16 B), the points for rank 0 first, then rank 1, ...;
 * d_counts (device, world + 2 words) receives the points per owner, then the slice's n_after_filter and n_in_map.
 * Enqueue-only on the engine's stream; the host reads d_counts to size the exchange (fdm_halo_route_exchange).
 * The plan: owned rect of rank i * grid_cols + j = rows [row_edge[i], row_edge[i+1]) x cols [col_edge[j], col_edge[j+1])
 * (fdm_tile_plan_route).  GLOBAL mode only, and raycasting off: an owner's ray stage would see only its own share, while
 * rays from every other point of the scan cross its cells, so the call fails with FDM_ERR_INVALID when the engine's
 * config has raycast_enabled set.
 *
 * fdm_engine_integrate_points4_device: FastDEM::integrate of the points an owner received ({x, y, z, intensity}
 * records in HBM, rank order = scan order).  any_in_map: some point of the LOGICAL scan landed in the map (the OR over
 * all slices' n_in_map) — it gates the obstacle-layer clear on every tile, also one that received no point. */
typedef struct fdm_route_plan {
  int32_t world, grid_rows, grid_cols, pad;
  int32_t row_edge[17], col_edge[17];
} fdm_route_plan;
int fdm_engine_route_scan(fdm_engine* e, const fdm_route_plan* plan, uint64_t n, const float* d_x, const float* d_y,
                          const float* d_z, const float* d_intensity, const double T_base_sensor[16],
                          const double T_world_base[16], float* d_send, uint32_t* d_counts);
int fdm_engine_integrate_points4_device(fdm_engine* e, uint64_t n, const float* d_points4, int has_intensity,
                                        int any_in_map, const double T_base_sensor[16],
                                        const double T_world_base[16]);
/* The same two halves with the shares laid out as CHANNEL BLOCKS (N scans, one per rank: every source's share is
 * integrated as a scan of its own, so nothing has to be contiguous across sources): the share of owner d starts at
 * float 4 * base_d of d_send, base_d = sum of pad4(count) over the lower owners, and holds x | y | z | intensity, each
 * pad4(count_d) floats.  A share is what the bin kernels read in place — no de-interleave pass on the receiving side,
 * the rank's own share is never copied.  d_send must hold 4 * (n + 3 * world) floats. */
int fdm_engine_route_scan_soa(fdm_engine* e, const fdm_route_plan* plan, uint64_t n, const float* d_x, const float* d_y,
                              const float* d_z, const float* d_intensity, const double T_base_sensor[16],
                              const double T_world_base[16], float* d_send, uint32_t* d_counts);
int fdm_engine_integrate_soa4_device(fdm_engine* e, uint64_t n, const float* d_share, int has_intensity,
                                     int any_in_map, const double T_base_sensor[16], const double T_world_base[16]);

/* Scan callbacks of the reference (fastdem.hpp:129-136, fastdem.cpp:139-150): when enabled the
 * kernels also keep (a) every point in the map frame + whether it survived the crops and (b) the
 * min-z observation of every observed cell.
 *   last_preprocessed: the cloud handed to onScanPreprocessed — points that survived cropRange and
 *     cropZ, in input order, map frame, with sigma_z2 = cov(2,2) (nullable).
 *   last_rasterized:   the cloud handed to onScanRasterized — one point per observed cell at the
 *     cell centre (GridMap::getPosition) with z = min_z (fastdem.cpp:200-214); order unspecified,
 *     as in the reference (hash-map iteration order).
 * Both return the number of points through n_out; `cap` is the capacity of the output arrays.
 * preprocessed == 2 also keeps the cloud's covariance channel (the reference's preprocessed cloud carries the
 * rotated 3x3 covariance of every point, nanopcl/core/point_cloud.hpp:126-147). */
int fdm_engine_capture(fdm_engine* e, int preprocessed, int rasterized);
/* The covariance channel of the preprocessed cloud: R * Sigma_sensor * R^T per surviving point
 * (fastdem.cpp:182-187), 9 floats per point, column-major like Eigen::Matrix3f, same order as
 * fdm_engine_last_preprocessed.  Needs fdm_engine_capture(e, 2, ..). */
int fdm_engine_last_preprocessed_cov(fdm_engine* e, uint64_t cap, float* cov9, uint64_t* n_out);
int fdm_engine_last_preprocessed(fdm_engine* e, uint64_t cap, float* x, float* y, float* z,
                                 float* sigma_z2, uint64_t* n_out);
int fdm_engine_last_rasterized(fdm_engine* e, uint64_t cap, float* x, float* y, float* z,
                               uint64_t* n_out);

/* ---- Raycasting stage ----
 * With cfg.raycast_enabled the integrate entry points also run step 3 of integrateImpl
 * (fastdem.cpp:152-159) on the device: sensor origin = (T_world_base*T_base_sensor).translation(),
 * voxelGrid(points, resolution, VoxelMode::ANY), applyRaycasting.  Layers `ghost_removal`,
 * `raycasting`, `_visibility_logodds` appear as in raycasting.cpp:223-226.  A resolution outside
 * voxelGrid's [0.001, 100] range makes integrate return FDM_ERR_INVALID (the reference throws,
 * voxel_grid_impl.hpp:31-33).
 *
 * fastdem::applyRaycasting(map, scan, sensor_origin, config) called directly
 * (postprocess/raycasting.hpp:47-49; tests/test_postprocess.cpp:73-190): `scan` is used as given,
 * no voxel filter.  rc == NULL takes the raycasting fields of the engine's fdm_config.  A no-op
 * when raycasting is disabled in that config, n == 0, or the sensor origin lies outside the map.
 * Host arrays, synchronous / device arrays, enqueue-only. */
int fdm_engine_apply_raycasting(fdm_engine* e, uint64_t n, const float* x, const float* y,
                                const float* z, const float sensor_origin[3],
                                const fdm_raycast_config* rc);
int fdm_engine_apply_raycasting_device(fdm_engine* e, uint64_t n, const float* d_x, const float* d_y,
                                       const float* d_z, const float sensor_origin[3],
                                       const fdm_raycast_config* rc);
/* nanopcl::filters::voxelGrid(cloud, voxel_size, VoxelMode::ANY) (voxel_grid_impl.hpp:30-60,171-189)
 * on the device: writes the ORIGINAL indices of the kept points, in the filter's output order
 * (ascending voxel key), to out_idx (capacity n) and their count to n_out.  Which point of a voxel
 * represents it follows the option "voxel_any_order": 0 (default) ties in original point order, 1 the order
 * libstdc++'s std::sort leaves — what a g++ build of the reference picks.
 * FDM_ERR_INVALID for a voxel_size outside [0.001, 100]. */
int fdm_engine_voxel_any(fdm_engine* e, uint64_t n, const float* x, const float* y, const float* z,
                         float voxel_size, uint32_t* out_idx, uint64_t* n_out);
/* HIP-event duration of the last scan's raycasting stage (keys + sort + rays + resolve), ms;
 * needs fdm_engine_enable_profile. */
int fdm_engine_last_ray_ms(fdm_engine* e, float* ms);

/* ---- Map egress ----
 * fastdem::detail::toPointCloud2Impl (bridge/ros/impl.hpp:28-166) on the device: one record per cell
 * with a finite `elevation_layer` value, in the reference's visiting order (column by column through
 * the submap, starting at sub_start), each record = x, y, z, every non-internal layer (name not
 * starting with '_', elevation_map.hpp:42-45) in getLayers() order, then the packed colour as `rgb`.
 * All fields are 4 bytes (FLOAT32): point_step = 4 * n_fields.  A record holds at most 64 float layers besides
 * x, y, z and rgb (67 fields, 68 with a `color` layer: point_step <= 272); a map with more visible layers is
 * refused with FDM_ERR_INVALID before anything is written (the reference has no such bound).
 *   sub_rows < 0 : the whole map (sub_start = start index, sub_size = size), impl.hpp:160-166
 *   fields_buf   : receives the field names separated by '\n' (nullable)
 *   host_out     : receives n_points * point_step bytes when cap_bytes allows; pass NULL (or a
 *                  too small cap) to learn n_points / point_step first
 * Compaction and packing run in HBM; the host sees one contiguous copy. */
int fdm_engine_pack_cloud(fdm_engine* e, const char* elevation_layer, int32_t sub_r0, int32_t sub_c0,
                          int32_t sub_rows, int32_t sub_cols, void* host_out, uint64_t cap_bytes,
                          uint64_t* n_points, uint32_t* point_step, char* fields_buf,
                          uint64_t fields_cap);
/* Same, the packed records stay in an engine-owned HBM buffer (valid until the next pack call). */
int fdm_engine_pack_cloud_device(fdm_engine* e, const char* elevation_layer, int32_t sub_r0,
                                 int32_t sub_c0, int32_t sub_rows, int32_t sub_cols, void** d_out,
                                 uint64_t* n_points, uint32_t* point_step);

/* ---- Layer images ----
 * The pixels of fastdem::io::savePng (io/png.hpp, src/io_png.cpp:115-171) computed on the device: one layer
 * -> row-major RGBA8, height = rows and width = cols of the stored window, 4 bytes per cell, a cell that is
 * not finite transparent black.  The normalisation range is computeRange's (io_png.cpp:32-65): the two
 * fixed numbers, min / max over the finite cells, or the order statistics of rank size_t(n * 0.01) and
 * min(size_t(n * 0.99), n - 1) of the n finite cells (one radix select for both, no sort); {0, 1} when no
 * cell is finite.  Pixels and range are exactly the reference's, bit for bit.
 * Mirrors fastdem::io::PngExportConfig field for field. */
typedef struct fdm_image_config {
  int32_t normalize;       /* Normalize: 0 MIN_MAX, 1 PERCENTILE_1_99, 2 FIXED_RANGE */
  int32_t colormap;        /* Colormap: 0 GRAYSCALE, 1 VIRIDIS, 2 JET */
  int32_t align_to_world;  /* != 0: unroll the circular buffer from the start index */
  float fixed_min, fixed_max;
} fdm_image_config;
void fdm_default_image_config(fdm_image_config* cfg);  /* PngExportConfig{}: PERCENTILE_1_99, VIRIDIS, aligned, -2 .. 2 */
/* host_rgba receives width * height * 4 bytes when cap_bytes allows; pass NULL (or a too small cap) to
 * learn width / height first — nothing is rendered then.  range2 (nullable) receives the {min, max} the
 * image was normalised with.  Any layer renders, internal ones ('_...') included; a missing layer is
 * FDM_ERR_NO_LAYER, an enum value out of range FDM_ERR_INVALID.  The map is not changed. */
int fdm_engine_render_layer(fdm_engine* e, const char* layer, const fdm_image_config* cfg,
                            void* host_rgba, uint64_t cap_bytes, int32_t* width, int32_t* height,
                            float range2[2]);
/* Same, the image stays in an engine-owned HBM buffer (valid until the next render call).  With
 * range2 == NULL the call only enqueues; asking for the range waits for it. */
int fdm_engine_render_layer_device(fdm_engine* e, const char* layer, const fdm_image_config* cfg,
                                   void** d_rgba, int32_t* width, int32_t* height, float range2[2]);

/* ---- Ingest ----
 * nanopcl::from(sensor_msgs::PointCloud2) (nanopcl/bridge/ros/impl.hpp:174-246) on the device.
 * The layout carries the byte offsets the reference parses from msg.fields (impl.hpp:65-99):
 * x, y, z are FLOAT32 and required; intensity (datatype UINT8=2, UINT16=4, FLOAT32=7, FLOAT64=8,
 * anything else reads as 0, impl.hpp:104-118) and rgb / rgba (packed 0x00RRGGBB, impl.hpp:163-171)
 * are optional: offset -1 = absent.  ring / time / label / normals are not consumed by integrate(). */
typedef struct fdm_cloud2_layout {
  uint32_t point_step;           /* msg.point_step */
  int32_t off_x, off_y, off_z;
  int32_t off_intensity, intensity_type;
  int32_t off_rgb;
} fdm_cloud2_layout;

/* from_impl: decode n_points records (msg.data, width*height of them) into the engine's SoA
 * channels in HBM, dropping points with a non-finite coordinate and keeping the order.
 * `data` is a host pointer (copied once) or, with data_on_device != 0, already in HBM.
 * n_valid receives the number of points kept (host sync). */
int fdm_engine_ingest_cloud2(fdm_engine* e, const void* data, int data_on_device, uint64_t n_points,
                             const fdm_cloud2_layout* layout, uint64_t* n_valid);
/* The channels the last ingest produced (device pointers, engine-owned, valid until the next
 * ingest): intensity / rgb are NULL when the message has no such field. */
int fdm_engine_ingested(fdm_engine* e, const float** d_x, const float** d_y, const float** d_z,
                        const float** d_intensity, const uint32_t** d_rgb, uint64_t* n);
/* from_impl + FastDEM::integrate(cloud, T_base_sensor, T_world_base) in one call (what the ROS
 * callback does, ros1/src/fastdem_ros_node.cpp:171-182).  Status as fdm_engine_integrate; a message
 * without x/y/z or whose points are all non-finite is an empty cloud (FDM_SKIP_EMPTY_CLOUD).
 * One decode kernel + the scan, no host round trip in between: the channels are written at the
 * message's indices, the bin kernel drops the non-finite points (the compaction from_impl does
 * changes indices, not decisions) and cloud.size() comes back with the scan statistics.  A message in
 * pinned memory (fdm_host_alloc) is decoded in place over PCIe; a pageable one is copied first. */
int fdm_engine_integrate_cloud2(fdm_engine* e, const void* data, int data_on_device, uint64_t n_points,
                                const fdm_cloud2_layout* layout, const double T_base_sensor[16],
                                const double T_world_base[16], fdm_scan_stats* out);

/* ---- Stencil post-processing ----
 * The reference's post-processing functions (called by the ROS timers on a snapshot of the map) on
 * the device-resident layers; each call only enqueues kernels.  Neighbourhoods are taken in logical
 * (unwrapped) coordinates and clipped at the map border; see DESIGN.md §7 f2 for the exact
 * neighbourhood definition (nanoGrid's region()/neighbors() are not on disk).  On a spatial tile the
 * stage is exact for the OWNED cells provided the halo ring is at least as wide as the stencil
 * reaches (inpainting: one cell per pass; median: kernel/2; the discs: radius/resolution) —
 * otherwise FDM_ERR_INVALID; halo cells must be refreshed from their owners afterwards
 * (fdm_engine_region_pack/_unpack).
 *   applyInpainting(map, max_iterations, min_valid_neighbors, inplace)        src/inpainting.cpp:21-67
 *   applySpatialSmoothing(map, layer, kernel_size, min_valid_neighbors)       postprocess/spatial_smoothing.hpp:38-67
 *   applyUncertaintyFusion(map, config::UncertaintyFusion)                    src/uncertainty_fusion.cpp:103-186
 *   applyFeatureExtraction(map, radius, min_valid, lower_pct, upper_pct)      src/feature_extraction.cpp:28-118
 * Any kernel size / radius the reference accepts is accepted: region(Size(k, k)) spans dr, dc in [-k/2, k/2] (for
 * an even k the (k + 1)-wide box); neighbourhoods beyond 256 cells (a 17 x 17 median, a 0.3 m disc
 * on a 0.02 m map) run through slower kernels whose per-cell lists live in a global pool and are insertion-sorted:
 * ~ entries^2 / 4 moves per cell.  A call whose neighbourhood would need more than ~1e13 moves over the map (minutes of
 * device time: 5 000 entries per cell at 1.44 M cells, 790 at 64 M) returns FDM_ERR_INVALID instead of hanging. */
typedef struct fdm_fusion_config {          /* config::UncertaintyFusion (config/postprocess.hpp:32-39) */
  int32_t enabled;
  float search_radius, spatial_sigma, quantile_lower, quantile_upper;
  int32_t min_valid_neighbors;
} fdm_fusion_config;
int fdm_engine_apply_inpainting(fdm_engine* e, int max_iterations, int min_valid_neighbors, int inplace);
int fdm_engine_apply_spatial_smoothing(fdm_engine* e, const char* layer, int kernel_size,
                                       int min_valid_neighbors);
int fdm_engine_apply_uncertainty_fusion(fdm_engine* e, const fdm_fusion_config* cfg);
int fdm_engine_apply_feature_extraction(fdm_engine* e, float analysis_radius, int min_valid_neighbors,
                                        float step_lower_percentile, float step_upper_percentile);

/* ---- static point clouds: fastdem/io/pcd_convert.hpp (src/pcd_convert.cpp:63-185, 327-373) ----
 * No sensor model, poses or estimator: a world-frame cloud is binned into the map as it stands (position and circular
 * start index included).  Per touched cell: elevation per `method` (0 Max, 1 Min, 2 Mean, 3 MinMax = RasterMethod),
 * elevation_min, elevation_max, variance (Welford in fp32 over the cell's points IN INPUT ORDER, m2 / (count - 1),
 * 0 for one point), n_points, intensity (the first value, then any strictly greater one) and color (the cell's last
 * point, 0x00RRGGBB) when the cloud has the channel.  A point with NaN z, or for which getIndex fails (outside, NaN
 * x / y), is skipped; an infinite z is not.  Missing layers are added in the reference's order (elevation_min,
 * elevation_max, variance, n_points, intensity, color); untouched cells keep what they held.  Works on map-only engines
 * and on engines with an estimator (record fields are written in place); a held-back map update is applied first.
 * Synchronous.  Returns FDM_SKIP_EMPTY_CLOUD for n == 0 and FDM_SKIP_NO_CELL when no point lands: nothing is written and
 * no layer is created.  FDM_ERR_INVALID: a tiled engine, n >= 2^31, an unknown method. */
typedef struct fdm_raster_stats {
  uint64_t n_points_used;    /* points that landed in a cell */
  uint64_t n_cells_written;  /* cells that received at least one */
} fdm_raster_stats;
/* SoA host arrays (intensity / rgb = 0x00RRGGBB nullable), staged by the engine; `out` may be NULL */
int fdm_engine_from_point_cloud(fdm_engine* e, uint64_t n, const float* x, const float* y, const float* z,
                                const float* intensity, const uint32_t* rgb, int method, fdm_raster_stats* out);
/* ... device arrays, read in place.  They must be complete when the call is made (it does not wait for other streams). */
int fdm_engine_from_point_cloud_device(fdm_engine* e, uint64_t n, const float* dx, const float* dy, const float* dz,
                                       const float* dintensity, const uint32_t* drgb, int method,
                                       fdm_raster_stats* out);
/* fromPointCloud(cloud, resolution, method): a map-only engine sized to the cloud's x / y bounding box (a min / max
 * reduction on the device over the points whose x and y are both non-NaN), then the call above.  In fp32 as the
 * reference: width = max_x - min_x + resolution (height likewise), position = ((min_x + max_x) / 2.0, (min_y + max_y) /
 * 2.0).  The arrays are host (on_device 0) or device arrays.  n == 0: FDM_SKIP_EMPTY_CLOUD and *out_engine = NULL (the
 * reference returns a map without geometry).  An extent that is not finite and positive (no point with both
 * coordinates, an infinite coordinate) is undefined in the reference and refused here with FDM_ERR_INVALID. */
int fdm_engine_create_from_point_cloud(uint64_t n, const void* x, const void* y, const void* z, const void* intensity,
                                       const void* rgb, int on_device, float resolution, int method, int device,
                                       fdm_engine** out_engine, fdm_raster_stats* out);
/* toPointCloud(map): one point per cell whose elevation is not NaN — x, y the cell centre (fp64 from the unwrapped index,
 * cast to float), z the elevation — in the visiting order of fdm_engine_pack_cloud over the whole map (unwrapped column by
 * column from the start index; nanoGrid's cells() order is ASSUMED to be that).  *has_intensity / *has_color: some emitted
 * cell holds a non-NaN intensity / colour (the reference's cloud has the channel exactly then); cells without one carry
 * 0.  Host arrays of `cap` points each (any may be NULL): *n_points is always the cloud's size; when that is more than
 * `cap` nothing is copied and the status is FDM_SKIP_BUFFER_TOO_SMALL. */
int fdm_engine_to_point_cloud(fdm_engine* e, uint64_t cap, float* x, float* y, float* z, float* intensity,
                              uint32_t* rgb, uint64_t* n_points, int32_t* has_intensity, int32_t* has_color);
/* ... the channels stay in an engine-owned device buffer, valid until the next call of either variant */
int fdm_engine_to_point_cloud_device(fdm_engine* e, const float** dx, const float** dy, const float** dz,
                                     const float** dintensity, const uint32_t** drgb, uint64_t* n_points,
                                     int32_t* has_intensity, int32_t* has_color);
/* with fdm_engine_enable_profile on: device ms of the last fromPointCloud's cell ids, grouping (sort) and walk */
int fdm_engine_last_raster_ms(fdm_engine* e, float* ms3);

/* ---- buildDEM: a clean DEM from a merged cloud (src/pcd_convert.cpp:194-323) and its two filter stages ----
 * Statistical outlier removal = nanopcl::filters::statisticalOutlierRemoval(cloud, k, std_mul)
 * (outlier_removal_impl.hpp:83-142).  effective_k = min(k, n - 1), a negative k counting as "every other point" (the
 * reference converts it to size_t).  Per point: the effective_k smallest squared distances to the OTHER points
 * (duplicates of the point count, at distance 0), each ((dx*dx) + (dy*dy)) + (dz*dz) in fp32 without contraction;
 * mean = (sum of their correctly rounded sqrt, ascending, fp32) / effective_k.  The global mean and the sum of squared
 * differences are fp64 sums in input order; threshold = float(mean) + std_mul * float(sqrt(ss / n)); keep[i] = mean[i]
 * <= threshold.  The search is EXACT k-NN; nanoflann's pruning bound is rounded and can miss a neighbour within
 * rounding of the k-th (ASSUMED equal otherwise: DESIGN.md §7).  k == 0, n == 0 and n == 1 keep nothing (*n_kept = 0,
 * FDM_OK).  FDM_ERR_INVALID: effective_k > 64; a coordinate that is NaN or infinite (undefined in the reference).
 * keep[n] and mean_dist[n] (nullable) are host arrays when the coordinates are (on_device 0), device arrays otherwise;
 * threshold and n_kept are host words.  Synchronous. */
int fdm_statistical_outlier_removal(uint64_t n, const float* x, const float* y, const float* z, int on_device, int k,
                                    float std_mul, int device, uint8_t* keep, float* mean_dist, float* threshold,
                                    uint64_t* n_kept);
/* what the calling thread's last outlier removal (the call above, or the one inside fdm_engine_build_dem) did */
typedef struct fdm_sor_stats {
  uint64_t n_queries;   /* points searched */
  uint64_t n_fallback;  /* ... of which the grid search left to the brute-force queue */
  int32_t grid_x, grid_y;  /* columns of the search grid */
  float voxel;          /* their edge, metres */
  float ms[4];          /* device ms: grid build, search, fallback queue, statistics (download and host sums included) */
} fdm_sor_stats;
int fdm_sor_last_stats(fdm_sor_stats* out);
/* removeFloatingPoints(cloud, map, height_threshold, bin) on e's geometry (pcd_convert.cpp:194-269): per cell a histogram
 * of z over bins of `bin` = bin_size > 0 ? bin_size : resolution from the cell's z_min, n_bins = max(1, int((z_max -
 * z_min) / bin) + 1), a point's bin min(int((z - z_min) / bin), n_bins - 1); the LOWEST bin with the largest count is
 * the ground; keep[i] = z <= (z_min + (best_bin + 0.5f) * bin) + height_threshold.  Points with NaN z or outside the
 * map are not kept.  FDM_ERR_INVALID: a cell whose (z_max - z_min) / bin does not fit an int32; a tiled engine.
 * keep[n] is a host array when the coordinates are (on_device 0), a device array otherwise.  The map is not touched. */
int fdm_engine_remove_floating_points(fdm_engine* e, uint64_t n, const float* x, const float* y, const float* z,
                                      int on_device, float height_threshold, float bin_size, uint8_t* keep,
                                      uint64_t* n_kept);
/* ---- cloud downsampling: nanopcl::filters::voxelGrid and gridMaxZ (filters/downsample.hpp; voxel_grid_impl.hpp:30-236,
 * grid_max_z_impl.hpp:31-75, core/voxel.hpp:28-102) ----
 * Engine-free and synchronous, on `device`.  The input is SoA: host arrays (on_device 0) or device arrays; x, y, z are
 * required, the other channels nullable, the normal's three arrays all or none.
 * KEYS AND ORDER.  inv = 1.0f / size; a point with a non-finite x, y or z is dropped; the others get the key
 * voxel::pack(x, y, z, inv): floor(v * inv) converted to int32 as x86 converts it (INT_MIN outside the int range),
 * clamped to [-2^20, 2^20 - 1], packed [z:21][y:21][x:21].  gridMaxZ packs (x, y, 0.0f) but still drops a point whose z
 * is not finite.  The (key, index) pairs are sorted by key and every run of equal keys gives one output point, in
 * ascending key order.  order 0: equal keys keep the input order (a stable sort); order 1: the order libstdc++'s
 * std::sort leaves them in, i.e. the reference's own (engine option "voxel_any_order").  `rep` is a run's first entry.
 * CENTROID (mode 0): x, y, z and intensity are fp32 sums from 0 over the run, in its order, each DIVIDED by
 * float(count); colour: float sums of r, g, b, each divided by the count and truncated to uint8; normal: component sums
 * s, norm = sqrt((sx*sx + sy*sy) + sz*sz) correctly rounded, s / norm if norm > 1e-6f, else (0, 0, 1); covariance: the
 * rep's.  CENTER (mode 3): the same, but the position is ((i + 0.5f) * size) per axis from the unpacked key.
 * NEAREST (mode 1): the point with the first strictly smallest d2 below FLT_MAX (the rep if none), d2 = (dx*dx + dz*dz)
 * + (dy*dy + 0) to that centre — the order of Eigen's 4-float packet reduction (ASSUMED: DESIGN.md §7); every channel is
 * that point's.  ANY (mode 2): entry start + (count * 7 + start * 13) % count of the sorted valid entries, `start` the
 * run's first — what fdm_engine_voxel_any picks.  gridMaxZ: the run's first strictly greatest z; every channel is
 * that point's.
 * OUTPUT.  Arrays of capacity n (the output is never larger than the input), host arrays for a host input and device
 * arrays otherwise; any may be NULL, and one whose input channel is absent is left untouched.  idx[r] = input index of
 * the point output r was copied from (CENTROID, CENTER: the run's rep), for the channels this ABI does not carry.
 * *n_out is a host word.  n == 0: FDM_OK, *n_out = 0.  FDM_ERR_INVALID: a size outside [0.001, 100] or NaN
 * ("voxel_size must be in [0.001, 100]" / "grid_size must be in [0.001, 100]"), an unknown mode or order,
 * n > 2^32 - 4097 (the sorts count tiles of 4 096 pairs in 32 bits), input normals given in part, a null x, y or z.
 * The thread's current device is put back before the call returns. */
typedef struct fdm_cloud_view {
  const float *x, *y, *z, *intensity;
  const uint32_t* rgb;          /* 0x00RRGGBB */
  const float *nx, *ny, *nz;    /* all three or none */
  const float* cov9;            /* 9 floats per point */
} fdm_cloud_view;
typedef struct fdm_cloud_out {
  float *x, *y, *z, *intensity;
  uint32_t* rgb;
  float *nx, *ny, *nz;
  float* cov9;
  uint32_t* idx;
} fdm_cloud_out;
/* mode: 0 CENTROID, 1 NEAREST, 2 ANY, 3 CENTER (VoxelMode's order) */
int fdm_cloud_voxel_grid(uint64_t n, const fdm_cloud_view* in, int on_device, float voxel_size, int mode, int order,
                         int device, const fdm_cloud_out* out, uint64_t* n_out);
int fdm_cloud_grid_max_z(uint64_t n, const fdm_cloud_view* in, int on_device, float grid_size, int order, int device,
                         const fdm_cloud_out* out, uint64_t* n_out);

/* ---- normals and GICP covariances of a cloud: nanopcl::geometry::estimateNormals, estimateCovariances and
 * estimateNormalsCovariances in their k-NN form (geometry/normal_estimation.hpp:43-63, 107-124, 159-179;
 * impl/normal_estimation_impl.hpp:33-68, impl/pca.hpp:34-107, impl/setters.hpp:20-105) ----
 * Engine-free and synchronous, on `device`; host arrays in and out (on_device 0) or device arrays.  Give nx, ny, nz (all
 * three or none), cov9 (9 floats per point, column-major), or both: both is the reference's single pass and equals the
 * two separate calls bit for bit.
 * NEIGHBOURS.  effective_k = min(size_t(k), n): a negative k means every point.  A point's neighbours are the
 * effective_k points of the whole cloud, ITSELF INCLUDED at distance 0, that are smallest by (d2, input index), d2 =
 * ((dx*dx) + (dy*dy)) + (dz*dz) in fp32 without contraction, d = query - point; they are taken in that order.  The
 * search is EXACT; nanoflann's pruning bound is rounded and can miss a neighbour within rounding of the k-th (ASSUMED
 * equal otherwise: DESIGN.md §7).  Where distances tie, nanoflann's order follows its tree traversal and cannot be
 * restated: the tie-break by input index is THIS PROJECT'S DEFINITION.
 * PCA.  Fewer than 3 neighbours (k in 0 .. 2, n < 3): invalid.  Otherwise offset = the first neighbour; sequential fp32
 * sums over the neighbours in order of d = p - offset and of d_a * d_b; inv_n = 1.0f / float(m); cov(a, b) = (sum_sq(a,
 * b) - (sum_a * sum_b) * inv_n) * inv_n (that reading of pca.hpp:55 ASSUMED: DESIGN.md §6); trace < FLT_EPSILON: invalid;
 * else Eigen's computeDirect, eigenvalues ascending, eigenvectors V.
 * OUTPUT.  normal = column 0 of V, negated when n . (viewpoint - p) < 0 (a dot of exactly 0 does not flip; viewpoint
 * NULL = the origin); an invalid normal is (0, 0, 0).  covariance = V diag(1e-3f, 1, 1) VT, V's columns scaled first
 * (ASSUMED, as the a0 b0 + (a1 b1 + a2 b2) order of every three-term dot: DESIGN.md §6); an invalid covariance is the
 * identity.  *n_invalid (nullable, a host word) = the points that got the invalid value.
 * n == 0: FDM_OK, nothing is touched.  FDM_ERR_INVALID: a coordinate that is NaN or infinite (looked for only where a
 * search runs, effective_k >= 3); effective_k > 64; normals given in part; neither normals nor cov9; n >= 2^31.  The
 * thread's current device is put back before the call returns. */
int fdm_cloud_estimate_normals(uint64_t n, const float* x, const float* y, const float* z, int on_device, int k,
                               const float viewpoint[3], int device, float* nx, float* ny, float* nz, float* cov9,
                               uint64_t* n_invalid);
typedef struct fdm_normal_stats {  /* the calling thread's last fdm_cloud_estimate_normals */
  uint64_t n_queries, n_fallback;  /* points searched; ... of which the grid search left to the brute-force queue */
  uint64_t n_invalid;              /* points that got the invalid value */
  int32_t grid_x, grid_y;          /* columns of the search grid */
  float voxel;                     /* their edge, metres */
  /* device ms while fdm_cloud_debug_profile (fdm_engine_debug.h) is on, zeros otherwise: grid build; search; fallback
   * queue; write.  The PCA is fused into the search and queue kernels, so `write` is what is left behind them: the
   * counters' read-back and a host cloud's download */
  float ms[4];
} fdm_normal_stats;
int fdm_normals_last_stats(fdm_normal_stats* out);

/* ---- registration of two clouds: nanopcl::registration::alignICP, alignPlaneICP and alignGICP (registration/align.hpp:
 * 71-246; iterative_solver.hpp:96-219, criteria.hpp:40-68, optimizers/lm_optimizer.hpp:98-103, linearizers/
 * linearizer.hpp:42-146, factors/{icp,plane,gicp}_factor.hpp, factors/robust_kernels.hpp:42-74, correspondence/
 * kdtree_correspondence.hpp:57-120, core/lie.hpp:39-148) ----
 * Engine-free and synchronous, on `device`; host arrays (on_device 0) or device arrays.  The per-iteration work — the
 * transform, the nearest target point within the radius, the factor and the sum of the factors — runs on the device; the
 * 6 x 6 algebra and the loop run on the host in double.  alignVGICP registers against a voxel distribution map built once:
 * fdm_voxel_map_create and fdm_cloud_register_vgicp, below.
 * LOOP.  T = initial_guess (16 doubles, column-major; NULL = the identity), prev_error = DBL_MAX, lambda = 1e-3 and never
 * adapted.  Per iteration: linearize every source point at T; fewer inliers than min_correspondences: failed (T, fitness
 * 0, rmse +inf, iterations = iter, not converged, no covariance); delta = (H + lambda I)^-1 (-b); new_T = se3Exp(delta) T;
 * converged: new_T with iter + 1; else T = new_T, prev_error = error.  After max_iterations: T, not converged, the last
 * model's statistics.  max_iterations <= 0: the initial guess, fitness 0, rmse +inf, 0 iterations.  An empty source or
 * target: the initial guess, 0, +inf, 0, not converged, before any channel is looked at.
 * delta is [v; omega]: se3Exp takes the first three as v and the last three as omega (so3Exp is the identity below
 * |omega| = 1e-10, else Rodrigues; t = leftJacobian(omega) v with c1 = (1 - cos) / theta, c2 = (theta - sin) / theta).
 * CONVERGENCE is criteria.hpp as written: |delta[3..5]| < translation_eps && |delta[0..2]| < rotation_eps — THE NAMES ARE
 * SWAPPED relative to that layout: translation_eps bounds the rotation part and rotation_eps the translation part.  Kept,
 * not corrected.  Converged also when rel_change < relative_error_eps, rel_change = prev > 0 ? |prev - curr| / prev : 0.
 * CORRESPONDENCE.  p = T * source[i] in double, ((r0 x + r1 y) + r2 z) + t per row without contraction (ASSUMED order:
 * DESIGN.md §6), rounded once to float; the nearest target point by d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32, d = p -
 * target; accepted iff d2 <= max_correspondence_dist * max_correspondence_dist (a float product).  Among equal distances
 * the LOWER TARGET INDEX wins: this project's definition (nanoflann's pick follows its tree).  The factor uses the double
 * p.  The search is exact.
 * FACTORS, all in double as written in the reference.  ICP has no robust kernel; plane ICP weights by |r|, GICP by the
 * Mahalanobis distance.  GICP regularises every covariance of both clouds once: cov(0, 0) not finite -> eps I; otherwise
 * V diag(eps, 1, 1) VT = I - (1 - eps) v0 v0T from the lower triangle cast to double, v0 the unit eigenvector of the
 * smallest eigenvalue, computed in double.  ASSUMED: an exactly diagonal input with equal diagonal gives diag(eps, 1, 1);
 * any other coincidence of the two smallest eigenvalues is unspecified.  The source's is rotated R C RT per iteration; W =
 * inverse3x3(C_src + C_tgt) by Cramer's rule.
 * RESULT.  fitness = inliers / n_source; rmse = sqrt(2 error / inliers) — unguarded on the converged path as in
 * makeSuccessResult, so converging on no inliers (min_correspondences 0, nothing in reach) gives NaN; the sums of the factors are taken in a fixed
 * tree (no atomics): two calls on the same input return the same bits.
 * DEVIATION.  The reference's covariance is Eigen's pivoted LDLT solve whenever isPositive(), which also holds for a
 * semidefinite H (plane ICP on a planar target: rank 3), with the near-zero pivots zeroed.  Here has_covariance = 1 only
 * when an unpivoted Cholesky in double of the last UNDAMPED H finds every pivot above n_source * 2^-52 * max diag(H);
 * covariance (row-major, [v; omega] order) is then inverse(H).  Otherwise it is absent.
 * FDM_ERR_INVALID: a coordinate of either cloud or an entry of the initial guess that is NaN or infinite; plane ICP
 * without all three target normal arrays; GICP without both cov9 arrays; a negative or NaN max_correspondence_dist; an
 * unknown method or kernel; n >= 2^31 in either cloud; a null x, y or z.  The thread's current device is put back before
 * the call returns. */
#define FDM_REGISTER_ICP 0
#define FDM_REGISTER_PLANE 1
#define FDM_REGISTER_GICP 2
typedef struct fdm_align_settings {  /* registration::AlignSettings (align.hpp:32-59), field for field */
  float max_correspondence_dist;     /* 1.0 */
  int32_t max_iterations;            /* 50 */
  double translation_eps;            /* 1e-4 */
  double rotation_eps;               /* 1e-4 */
  double relative_error_eps;         /* 1e-6 */
  uint64_t min_correspondences;      /* 10 */
  int32_t robust_kernel;             /* RobustKernel: 0 NONE, 1 HUBER, 2 TUKEY, 3 CAUCHY (plane ICP and GICP) */
  int32_t reserved;
  double robust_kernel_width;        /* 1.0 */
  double covariance_epsilon;         /* 1e-3 (GICP) */
} fdm_align_settings;
void fdm_default_align_settings(fdm_align_settings* settings);
typedef struct fdm_register_clouds {
  uint64_t n_source;
  const float *sx, *sy, *sz;
  const float* s_cov9;               /* GICP: 9 floats per point, column-major; else NULL */
  uint64_t n_target;
  const float *tx, *ty, *tz;
  const float *tnx, *tny, *tnz;      /* plane ICP: all three; else NULL */
  const float* t_cov9;               /* GICP */
  int32_t on_device;                 /* 0: host arrays, else device arrays */
} fdm_register_clouds;
typedef struct fdm_registration_result {  /* registration::RegistrationResult (result.hpp:27-60) */
  double transform[16];              /* column-major, source -> target */
  double fitness, rmse;
  uint64_t iterations;
  int32_t converged, has_covariance;
  double covariance[36];             /* valid when has_covariance */
} fdm_registration_result;
/* method: FDM_REGISTER_ICP, _PLANE or _GICP; settings NULL = the defaults */
int fdm_cloud_register(int method, const fdm_register_clouds* clouds, const double* initial_guess,
                       const fdm_align_settings* settings, int device, fdm_registration_result* out);
/* One linearization at `transform` (NULL = the identity) — the reference's linearizer: H[21] (upper triangle, row-major),
 * b[6], the error and the inlier count.  corr (nullable; n_source int32, a host array for host clouds and a device array
 * otherwise) receives the target index each source point corresponds to, -1 for none.  An empty cloud gives zeros. */
int fdm_cloud_register_linearize(int method, const fdm_register_clouds* clouds, const double* transform,
                                 const fdm_align_settings* settings, int device, double H[21], double b[6], double* error,
                                 uint64_t* num_inliers, int32_t* corr);
typedef struct fdm_register_stats {  /* the calling thread's last fdm_cloud_register / fdm_cloud_register_linearize */
  uint64_t n_source, n_target;
  int32_t grid_x, grid_y;            /* columns of the target's search grid */
  float voxel;                       /* their edge, metres */
  int32_t ring_limit;                /* rings a query may visit: those that cover the radius, capped by the grid */
  int32_t linearizations;            /* linearize launches */
  /* device ms while fdm_cloud_debug_profile (fdm_engine_debug.h) is on, zeros otherwise (no events are created then):
   * the grid build; the regularisation of both clouds' covariances; the linearizations (search, factor and sums), summed */
  float ms[3];
} fdm_register_stats;
int fdm_register_last_stats(fdm_register_stats* out);

/* ---- voxelized GICP: nanopcl::registration::VoxelDistributionMap, VoxelCorrespondence and alignVGICP (registration/
 * voxel_distribution_map.hpp:143-323, correspondence/voxel_correspondence.hpp:35-78, factors/vgicp_factor.hpp,
 * align.hpp:276-353, core/voxel.hpp:28-42) ----
 * The target is turned ONCE into a map of per-voxel means and covariances; every later scan is registered against it with
 * one table lookup per source point and iteration, where GICP searches for a nearest neighbour.  A map owns device memory
 * on one device, outlives the call that made it and may serve any number of register calls; it is not changed by them.
 * BUILD.  inv = 1.0f / resolution.  A target point with a non-finite x, y or z is SKIPPED (counted in n_skipped), as in
 * the reference; every other point gets the key fdm_cloud_voxel_grid documents (voxel::pack: the float product, floor, the
 * x86 int conversion, the clamp to [-2^20, 2^20 - 1], [z:21][y:21][x:21]).  Per key, in INPUT ORDER and in double: sum of
 * p and sum_outer of p_a * p_b (exact products of two floats), the first point of a voxel ASSIGNED and the others added —
 * a voxel whose points all have x = -0.0f keeps a -0.0 sum — sequentially, without reassociation or atomics; count is a
 * uint32.  mean = sum / double(count), stored as float.  count >= 3: cov(a, b) = sum_outer(a, b) / double(count) - mean_a *
 * mean_b in double without contraction, stored as float.  count 1 or 2: cov = float(covariance_epsilon) * I.
 * VOXEL ORDER (this project's definition).  Records, and the indices a correspondence names, are in ASCENDING KEY order;
 * the reference's table order is not observable through its API.
 * REGULARISED COVARIANCE.  C_reg of a voxel of count >= 3 is I - (1 - eps) v0 v0T computed in DOUBLE from the stored float
 * covariance (lower triangle), v0 the unit eigenvector of its smallest eigenvalue, and kept in double: the arithmetic GICP
 * applies to a point's covariance, above.  C_reg of a sparser voxel is exactly I.  DEVIATION: the reference reaches the
 * same matrix through a float eigen-solver and float products and casts the result to double; the two differ at float
 * rounding.  Where the two smallest eigenvalues of a voxel's covariance coincide (three collinear points, repeated
 * points) v0 is unspecified there and here.
 * LOOKUP.  The voxel of a point is the record of its key; a voxel that exists is always valid (count >= 1).  The table is
 * open addressing over the distinct keys, a power of two of at least 2 * num_voxels slots, the first slot a mix of all 63
 * key bits; a lookup probes at most max_probe slots, the longest sequence the build took.
 * ALIGN.  As fdm_cloud_register with GICP's factor, loop, convergence, result and covariance rule, except: the
 * correspondence of source point i is the voxel of p = T * source[i] cast to float — no voxel, no correspondence;
 * max_correspondence_dist is NOT USED; q = double(mean), C_tgt = the voxel's C_reg, C_src = R C_reg_src RT with the
 * source's covariances regularised once with settings->covariance_epsilon.  An empty source or an empty map returns the
 * early result (the guess, 0, +inf, 0, not converged) before anything else is looked at; a source without covariances is
 * refused ("alignVGICP: source must have covariances").  The convenience overload alignVGICP(source, target,
 * voxel_resolution, ...) is a map built with settings->covariance_epsilon, one register call and the map's destruction.
 * FDM_ERR_INVALID: a resolution or 1.0f / resolution that is not finite and > 0; a negative or NaN covariance_epsilon; a
 * source coordinate that is not finite (undefined in the reference: the cast to int); n_target > 2^32 - 4097 (the sorts'
 * limit); n_source >= 2^31; device source arrays that live on another device than the map; an entry of the transform that
 * is not finite; an unknown robust kernel; a null argument.  The thread's current device is put back before every call
 * returns.  The build's scratch is freed before fdm_voxel_map_create returns: a map keeps its records and its table. */
typedef struct fdm_voxel_map fdm_voxel_map;   /* opaque; owns device memory on one device */
typedef struct fdm_voxel_map_info {
  float resolution, inv_resolution;
  double covariance_epsilon;
  int32_t device, reserved;
  uint64_t n_points, n_skipped;      /* points given; ... of which not finite */
  uint64_t num_voxels, n_sparse;     /* distinct keys; ... of which with fewer than 3 points */
  uint64_t table_slots;              /* 0 for an empty map */
  uint32_t max_count, max_probe;     /* the fullest voxel's points; slots the longest insertion looked at */
  /* device ms while fdm_cloud_debug_profile (fdm_engine_debug.h) was on at the build, zeros otherwise: keys and sort;
   * run heads, reduction and regularisation; the table */
  float ms[3];
  float reserved2;
} fdm_voxel_map_info;
/* x, y, z: host arrays (on_device 0) or device arrays on `device`.  n == 0 or no finite point: an empty map. */
int fdm_voxel_map_create(uint64_t n, const float* x, const float* y, const float* z, int on_device, float resolution,
                         double covariance_epsilon, int device, fdm_voxel_map** out);
void fdm_voxel_map_destroy(fdm_voxel_map* map);   /* NULL is fine */
int fdm_voxel_map_get_info(const fdm_voxel_map* map, fdm_voxel_map_info* out);
/* The records in ascending key order, num_voxels entries each, into host arrays (on_device 0) or device arrays on the
 * map's device; any may be NULL.  mean3: 3 floats; cov9: 9 floats, column-major; creg6: xx, xy, xz, yy, yz, zz. */
int fdm_voxel_map_records(const fdm_voxel_map* map, int on_device, uint64_t* keys, float* mean3, float* cov9,
                          double* creg6, uint32_t* count);
/* alignVGICP(source, correspondence, initial_guess, settings) on the map's device.  fdm_register_last_stats afterwards:
 * n_target = num_voxels, grid_x = grid_y = ring_limit = 0, voxel = the resolution, ms[0] = 0 (the map was built
 * elsewhere), ms[1] the source's regularisation, ms[2] the linearizations. */
int fdm_cloud_register_vgicp(const fdm_voxel_map* map, uint64_t n_source, const float* sx, const float* sy,
                             const float* sz, const float* s_cov9, int on_device, const double* initial_guess,
                             const fdm_align_settings* settings, fdm_registration_result* out);
/* One linearization at `transform` (NULL = the identity), as fdm_cloud_register_linearize; corr[i] = the rank in
 * ascending key order of the voxel source point i corresponds to, -1 for none.  An empty source or map gives zeros. */
int fdm_cloud_register_vgicp_linearize(const fdm_voxel_map* map, uint64_t n_source, const float* sx, const float* sy,
                                       const float* sz, const float* s_cov9, int on_device, const double* transform,
                                       const fdm_align_settings* settings, double H[21], double b[6], double* error,
                                       uint64_t* num_inliers, int32_t* corr);

/* ---- cloud segmentation: nanopcl::segmentation::segmentGround (segmentation/impl/ground_seg_impl.hpp:27-123) and
 * segmentPlane / segmentMultiplePlanes (RANSAC; segmentation/impl/ransac_plane_impl.hpp:29-405) ----
 * Engine-free and synchronous, on `device`; host arrays (on_device 0) or device arrays, the outputs where the inputs
 * are; counts and results are host words.  The thread's current device is put back before a call returns.  All fp32
 * arithmetic is done without contraction.  euclideanCluster: fdm_cloud_cluster, below.
 *
 * SEGMENT GROUND (:68-112).  A point's cell is gx = int(floor(x / grid_resolution)), gy likewise: a correctly rounded
 * fp32 DIVISION (:33-34), not a product with a reciprocal.  A cell of fewer than min_points_per_cell points is
 * obstacle-only (:46-48).  Otherwise its z values are sorted ascending, idx = size_t(cell_percentile * float(count - 1))
 * — a float product, truncated — idx = min(idx, count - 1), robust = z_sorted[idx] (:54-57); robust > max_ground_height
 * makes the cell obstacle-only (:60-62).  A point of another cell is an obstacle iff z > robust + ground_thickness, a
 * strict comparison with an fp32 sum (:100-102).  ground and obstacles (capacity n each, either may be NULL) receive the
 * point indices in ascending order; together they hold every point once.  n == 0: FDM_OK, both counts 0.
 * FDM_ERR_INVALID, where the reference is undefined, with the lists untouched: a coordinate that is not finite; a floor
 * outside int32; a resolution that is not finite and > 0; a percentile that is NaN or < 0 (one > 1 is clamped by the
 * min, as in the reference); n > 2^32 - 4097 (the sorts' limit); a null x, y or z. */
typedef struct fdm_ground_seg_config {  /* GroundSegConfig (segmentation/ground_seg.hpp), field for field */
  float grid_resolution;                /* 0.5 */
  float cell_percentile;                /* 0.2 */
  float ground_thickness;               /* 0.3 */
  float max_ground_height;              /* 0.5 */
  uint64_t min_points_per_cell;         /* 2 */
} fdm_ground_seg_config;
/* cfg NULL = the defaults */
int fdm_cloud_segment_ground(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                             const fdm_ground_seg_config* cfg, int device, uint32_t* ground, uint32_t* obstacles,
                             uint64_t* n_ground, uint64_t* n_obstacles);

/* SEGMENT PLANE (:241-334) over the index list (`indices` NULL = every point, in order; n_indices is then ignored and n
 * is used).  XorShift64(42) is restarted on every call (:251); an iteration draws three POSITIONS in the list, then
 * redraws the second while it equals the first and the third while it equals either (:265-273); the draws never depend
 * on the model.  PlaneModel::fromPoints (:196-215): v1 = p2 - p1, v2 = p3 - p1, n = v1 x v2 as Eigen writes the cross
 * product, norm = sqrt(n0*n0 + (n1*n1 + n2*n2)) correctly rounded (the three-term order ASSUMED: DESIGN.md §6); norm <
 * 1e-10f: invalid; else n /= norm, d = -(n0*p1x + (n1*p1y + n2*p1z)); a model is valid iff d is finite, so a sampled NaN
 * or infinite point gives an invalid model.  A point is an inlier iff |((nx*px + ny*py) + nz*pz) + d| < distance_threshold
 * (:91).  A strictly greater count replaces the best and sets adaptive = computeAdaptiveIterations(count / double(n_indices),
 * probability) in double (:56-71; a value no int holds is saturated); the loop ends at iter >= min(max_iterations,
 * adaptive).  The engine scores the hypotheses of `batch` iterations per launch and replays the loop on the host over
 * their counts in order: it stops at the exact iteration the sequential code stops at, and nothing computed past it
 * influences the result.
 * The default result — coefficients (0, 0, 1, 0), no inliers, fitness 0, iterations 0, success 0 — is returned for
 * n_indices < 3 (:247) and for a best count below min_inliers (:310).  Otherwise the inliers of the best model are
 * collected in list order; with refine_model and >= 3 of them the model is refined (:134-188) and, the refined model
 * being valid, the inliers are collected again with it; fitness = n_inliers / double(n_indices); iterations = the loop
 * passes made; success = the list is not empty.
 * REFINEMENT.  The centroid in double, then the six central second moments in double about it, the symmetric 3 x 3
 * eigenproblem in double, the eigenvector of the smallest eigenvalue cast to float and normalized in fp32, d = -(n .
 * float(centroid)) in the three-term order.  Two things cannot be restated.  SUMMATION ORDER: the engine's sums are a
 * fixed tree — the same for the same inlier count, no floating-point atomics — and differ from the reference's
 * sequential sums by at most the rounding of n_inliers double additions.  EIGENVECTOR SIGN: Eigen's follows its QL
 * iteration; THIS PROJECT'S DEFINITION: the refined normal's dot with the unrefined best model's normal (the float
 * products summed in double) is not negative, and where it is exactly 0 the first non-zero component is positive.
 * inliers: capacity n_indices (n for a NULL list).  FDM_ERR_INVALID: n >= 2^32; a list — or, without one, a cloud — of
 * more than 2^32 - 4097 entries (blocks of 256 list positions are counted in 32 bits); an index >= n —
 * found by a pass that only reads the list, before any kernel uses an entry as an address; a threshold that is NaN; a
 * null x, y, z, inliers or result. */
typedef struct fdm_ransac_config {  /* RansacConfig (segmentation/ransac_plane.hpp), field for field */
  float distance_threshold;         /* 0.1 */
  int32_t max_iterations;           /* 1000 */
  double probability;               /* 0.99 */
  uint64_t min_inliers;             /* 3 */
  int32_t refine_model;             /* 1 */
} fdm_ransac_config;
typedef struct fdm_ransac_result {
  float coefficients[4];            /* nx, ny, nz, d */
  double fitness;
  int32_t iterations;
  int32_t success;
  uint64_t n_inliers;
} fdm_ransac_result;
/* cfg NULL = the defaults */
int fdm_cloud_segment_plane(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                            const uint32_t* indices, uint64_t n_indices, const fdm_ransac_config* cfg, int device,
                            uint32_t* inliers, fdm_ransac_result* result);
/* segmentMultiplePlanes (:366-405): the list of remaining indices starts as every point and stays on the device; after
 * each accepted plane its inliers are struck out, the order of the rest kept.  The loop ends at max_planes, at fewer
 * than 3 remaining indices, or at the first result without success or with fitness < min_fitness, which is not
 * returned.  inliers (capacity n) receives the planes' lists one after the other, results[max_planes] their results,
 * *n_planes how many. */
int fdm_cloud_segment_planes(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                             const fdm_ransac_config* cfg, uint64_t max_planes, double min_fitness, int device,
                             uint32_t* inliers, fdm_ransac_result* results, uint64_t* n_planes);
typedef struct fdm_segment_stats {  /* the calling thread's last segmentation call (of segment_planes: summed over its planes) */
  uint64_t n_batches;               /* launches of the scoring kernel */
  uint64_t n_hypotheses;            /* hypotheses they scored, those past the loop's stop included */
  uint64_t n_invalid_samples;       /* loop passes whose sample gave no valid model */
  uint32_t batch;                   /* iterations per launch */
  /* device ms while fdm_cloud_debug_profile (fdm_engine_debug.h) is on, zeros otherwise.  segment_plane(s): models and
   * scoring, summed; collecting; the refinement's sums; the strike-out.  segment_ground: keys; the two sorts; run heads,
   * cuts and classification; the two compactions */
  float ms[4];
} fdm_segment_stats;
int fdm_segment_last_stats(fdm_segment_stats* out);

/* ---- Euclidean clustering: nanopcl::segmentation::euclideanCluster (segmentation/impl/euclidean_cluster_impl.hpp:89-225
 * over search/impl/voxel_hash_impl.hpp:118-161 and core/voxel.hpp:28-80) ----
 * Engine-free and synchronous like the segmentation calls; host arrays (on_device 0) or device arrays, the outputs
 * where the cloud is; *n_clusters is a host word.  The list is `indices` (n_indices entries) or, for NULL, every point in
 * order; m = its length.  A "position" is a position in the list; a duplicate entry is two points.
 * THE RELATION, restated exactly.  inv = 1.0f / tolerance, range = int(ceil(tolerance * inv)) (1 for every tolerance
 * tried; 2 is handled), r_sq = tolerance * tolerance, in fp32.  A point's voxel is floor(c * inv) per axis: the fp32
 * PRODUCT, not segment_ground's division.  Two listed points are neighbours iff their voxels differ by at most `range`
 * on every axis (part of the relation: the voxels the reference's radius search visits) and dist_sq <= r_sq, where
 * dist_sq = dx*dx + (dy*dy + dz*dz) of the fp32 differences, without contraction: the three-term order of DESIGN.md §6,
 * FIXED here (the reference's is its compiler's).  The clusters are the connected components of that relation; a
 * component is kept iff min_size <= size <= max_size (an oversized one is dropped whole).
 * THE ORDER, this project's definition: kept clusters in descending size, clusters of equal size by their smallest
 * position ascending; inside a cluster ascending position.  The reference takes its seeds in ascending index, so its
 * clusters exist in ascending order of their smallest member before its final std::sort by size: this is that sort read
 * as a STABLE one.  (The reference's order inside a cluster is its BFS order over hash chains; it is not reproduced.)
 * The sequence of sizes equals the reference's, every cluster equals a reference cluster as a set, and a cluster's
 * first element is the reference's seed.
 * OUTPUT: CSR.  cluster_indices (capacity m) holds the list's ENTRIES — indices into the cloud — cluster after cluster;
 * offsets (capacity m + 1) holds n_clusters + 1 words, offsets[0] = 0; labels (NULL, or capacity m) gets per position 0
 * (in no kept cluster) or its cluster's number + 1.  m == 0: FDM_OK, *n_clusters = 0, offsets[0] = 0.
 * FDM_ERR_INVALID, with the outputs untouched: a listed coordinate that is not finite (the reference casts it to int);
 * a voxel coordinate outside [-2^20 + range, 2^20 - 1 - range] (the reference clamps it: its table degenerates); a
 * tolerance that is <= 0, NaN or infinite, or whose range is not 1 or 2; an entry >= n (found by a pass that reads the
 * list alone, before any kernel addresses with an entry); n >= 2^32; m >= 2^32 - 4097; a null x, y, z, offsets or (m > 0)
 * cluster_indices; MORE THAN 1.5e11 CANDIDATE PAIRS — the sum over the points of the points at a lower sorted position in
 * the voxels they search, which is the work of the merge as it is of the reference's search: a voxel of c points costs
 * c^2 / 2.  The bound is 0.6 - 1.1 s of the MI355X (measured: profiles/r13/cluster/README.md); the call returns instead
 * of running for longer.  No kernel of this call waits on another block, and every loop of its union-find is counted: a find
 * that does not end within m steps or a unite that loses its swap 4096 times returns FDM_ERR_HIP with its message. */
typedef struct fdm_cluster_config {  /* ClusterConfig (segmentation/euclidean_cluster.hpp), field for field */
  float tolerance;                   /* 0.5 */
  uint64_t min_size;                 /* 10 */
  uint64_t max_size;                 /* 100000 */
} fdm_cluster_config;
/* cfg NULL = the defaults */
int fdm_cloud_cluster(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                      const uint32_t* indices, uint64_t n_indices, const fdm_cluster_config* cfg, int device,
                      uint32_t* cluster_indices, uint32_t* offsets, uint32_t* labels, uint64_t* n_clusters);
typedef struct fdm_cluster_stats {   /* the calling thread's last fdm_cloud_cluster */
  uint64_t n_points;                 /* m */
  uint64_t n_components;             /* connected components; n_kept + n_rejected */
  uint64_t n_kept;                   /* = *n_clusters */
  uint64_t n_rejected;               /* below min_size or above max_size */
  uint64_t n_clustered;              /* points in kept clusters */
  uint64_t candidate_pairs;          /* the work bound's measure */
  uint64_t tests;                    /* distance tests made: every candidate pair once */
  uint64_t neighbour_pairs;          /* of them within the tolerance */
  uint64_t unions;                   /* links made: n_points - n_components */
  int32_t range;
  uint32_t key_bits;                 /* of the voxel key over the bounding box */
  /* device ms while fdm_cloud_debug_profile (fdm_engine_debug.h) is on, zeros otherwise: checks and voxels; keys, sort
   * and gather; candidate intervals; merge; roots, sizes and the kept positions; ordering sort, offsets, indices, labels */
  float ms[6];
} fdm_cluster_stats;
int fdm_cluster_last_stats(fdm_cluster_stats* out);

/* ---- Cloud filters: nanopcl::filters::radiusOutlierRemoval (filters/impl/outlier_removal_impl.hpp:21-77 over
 * search/impl/voxel_hash_impl.hpp:13-64, :118-161), the crop family (filters/impl/crop_impl.hpp) and removeInvalid
 * (filters/core.hpp:95-109) ----
 * Engine-free and synchronous like the clustering call; host arrays (on_device 0) or device arrays, keep (n bytes, 1 =
 * the point stays) and counts (NULL, or n words) where the cloud is; *n_kept is a host word.  A call selects, it never
 * moves a point: the caller compacts with the mask.
 * RADIUS OUTLIER REMOVAL.  The relation is fdm_cloud_cluster's, with inv = 1.0f / radius, r_sq = radius * radius and
 * range = int(ceil(radius * inv)) in fp32: count[i] = the number of j != i — by INDEX, so a duplicate coordinate counts —
 * whose voxels floor(c * inv) differ from i's by at most `range` on every axis and whose dist_sq = dx*dx + (dy*dy + dz*dz)
 * <= r_sq, the three-term order of DESIGN.md §6 without contraction (ASSUMED, as for clustering: the reference's order is
 * its compiler's).  keep[i] = count[i] >= min_neighbors; min_neighbors == 0 keeps every point.  counts NULL is MASK
 * MODE: a point's search stops once it has min_neighbors neighbours, its own voxel row first; with counts the whole
 * neighbourhood is walked and the exact count written.  Both give the same keep.  n == 0: FDM_OK, *n_kept = 0.
 * FDM_ERR_INVALID, with the outputs untouched: a coordinate that is not finite (the reference casts it to int:
 * fdm_cloud_crop with FDM_CROP_FINITE removes such points first); a voxel coordinate outside [-2^20 + range, 2^20 - 1 -
 * range] (the reference clamps it: its table degenerates); a radius that is <= 0, NaN or infinite, or whose range is not
 * 1 or 2; n >= 2^32 - 4097; a null x, y, z, keep or n_kept; MORE THAN 1.5e11 CANDIDATE TESTS — the sum over the points of
 * the other points in the voxels they search, the work of count mode as it is of the reference's search: a voxel of c
 * points costs c^2.  The bound's measurement is in profiles/r20/filters/README.md; the call returns instead of running for
 * longer, in either mode. */
int fdm_cloud_radius_outlier_removal(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                                     float radius, uint64_t min_neighbors, int device,
                                     uint8_t* keep, uint32_t* counts, uint64_t* n_kept);
typedef struct fdm_ror_stats {       /* the calling thread's last fdm_cloud_radius_outlier_removal */
  uint64_t n_points;
  uint64_t candidate_tests;          /* the work bound's measure */
  uint64_t tests_done;               /* distance tests made: candidate_tests in count mode, fewer in mask mode */
  uint64_t n_kept;                   /* = *n_kept */
  int32_t range;
  uint32_t key_bits;                 /* of the voxel key over the bounding box */
  /* device ms while fdm_cloud_debug_profile (fdm_engine_debug.h) is on, zeros otherwise: checks and voxels; keys, sort
   * and gather; candidate tests; the count kernel; the outputs' way back */
  float ms[5];
} fdm_ror_stats;
int fdm_ror_last_stats(fdm_ror_stats* out);

/* THE PREDICATE FILTERS, each written as the reference writes it, comparison by comparison — which fixes what a NaN does:
 * an axis crop drops a NaN coordinate in both modes, cropBox OUTSIDE keeps a point with a NaN x whose y lies outside,
 * cropAngle OUTSIDE keeps what INSIDE's expression calls false.  min > max is not refused (the reference does not).
 *   BOX     INSIDE: lo[k] <= c[k] <= hi[k] on every axis; OUTSIDE: c[k] < lo[k] or c[k] > hi[k] on some axis
 *   RANGE   d2 = x*x + (y*y + z*z) against lo[0] * lo[0] and hi[0] * hi[0], all fp32 (squaredNorm's order: ASSUMED, §6)
 *   X, Y, Z the coordinate against lo[0] and hi[0]
 *   ANGLE   min = lo[0], max = hi[0] in radians: c = cos * y - sin * x per angle, each product and the difference rounded
 *           to fp32 (the product form: ASSUMED), against eps = 1e-5f; in_range = (c_min >= -eps AND / OR c_max <= eps), AND
 *           iff the span — 2.0f * float(M_PI) - (min - max) for min > max, else max - min — is below float(M_PI); the four
 *           constants are the host's cosf / sinf
 *   FINITE  removeInvalid: every coordinate finite; `mode` is not read
 * FDM_ERR_INVALID: a kind or mode not listed, a null cfg, x, y, z, keep or n_kept, n >= 2^32. */
#define FDM_CROP_BOX 0
#define FDM_CROP_RANGE 1
#define FDM_CROP_X 2
#define FDM_CROP_Y 3
#define FDM_CROP_Z 4
#define FDM_CROP_ANGLE 5
#define FDM_CROP_FINITE 6
#define FDM_CROP_INSIDE 0
#define FDM_CROP_OUTSIDE 1
typedef struct fdm_crop_config {
  int32_t kind;                      /* FDM_CROP_BOX .. FDM_CROP_FINITE */
  int32_t mode;                      /* FilterMode: FDM_CROP_INSIDE, FDM_CROP_OUTSIDE */
  float lo[3], hi[3];
} fdm_crop_config;
int fdm_cloud_crop(uint64_t n, const float* x, const float* y, const float* z, int on_device,
                   const fdm_crop_config* cfg, int device, uint8_t* keep, uint64_t* n_kept);

typedef struct fdm_dem_config {  /* fastdem::DEMConfig (io/pcd_convert.hpp:28-42), field for field */
  float resolution;
  int32_t method;              /* RasterMethod: 0 Max, 1 Min, 2 Mean, 3 MinMax */
  int32_t sor_k;
  float sor_std_mul;
  float height_threshold;
  float bin_size;              /* 0 = the resolution */
  int32_t inpaint_iterations;  /* 0 = no inpainting */
} fdm_dem_config;
void fdm_default_dem_config(fdm_dem_config* cfg);  /* 0.1, Max, 10, 1.0, 2.0, 0.0, 3 */
typedef struct fdm_dem_stats {
  uint64_t n_input, n_after_sor, n_after_height;
  uint64_t n_sor_fallback;   /* queries of the outlier removal that took the brute-force queue */
  float sor_threshold;
  float stage_ms[7];         /* device ms: k-NN grid build, search, fallback queue, statistics, height filter, raster, inpaint */
  fdm_raster_stats raster;
} fdm_dem_stats;
/* buildDEM(cloud, config): outlier removal, a map over the survivors' x / y bounding box (sized as
 * fdm_engine_create_from_point_cloud sizes it), floating-point removal on that map, fromPointCloud with `method`,
 * applyInpainting(map, inpaint_iterations, 2, inplace) when inpaint_iterations > 0.  The cloud stays on the device
 * between the stages; the survivors keep their input order, intensity and colour.  cfg NULL = the defaults.  The result
 * is a map-only engine.  FDM_SKIP_EMPTY_CLOUD (n == 0) and FDM_SKIP_ALL_FILTERED (the outlier removal keeps nothing:
 * one point, sor_k == 0) leave *out_engine NULL, where the reference returns a map without geometry. */
int fdm_engine_build_dem(uint64_t n, const void* x, const void* y, const void* z, const void* intensity,
                         const void* rgb, int on_device, const fdm_dem_config* cfg, int device,
                         fdm_engine** out_engine, fdm_dem_stats* stats);

/* PCD files: nanopcl::io::loadPCD / savePCD (nanopcl/io/pcd_io.hpp:243-378, :415-550) and the two calls of the pcd2dem
 * tool (fastdem/tools/pcd2dem.cpp).  The header and ASCII records are host work; binary records are decoded and packed
 * on the device, so a file's bytes cross PCIe once and the cloud never exists on the host as arrays. */
#define FDM_PCD_ASCII 0
#define FDM_PCD_BINARY 1
#define FDM_PCD_MAX_FIELDS 64
typedef struct fdm_pcd_field {  /* detail::PCDFieldInfo (:72-78) */
  char name[64];                /* lower-cased, NUL-terminated (a longer name is cut: it matches no channel) */
  char type;                    /* the TYPE token's first character as written: F, U, I or anything else */
  uint8_t reserved[3];
  uint32_t size, count, offset; /* offset: the running sum of size * count, uint32 arithmetic */
} fdm_pcd_field;
typedef struct fdm_pcd_header {  /* detail::PCDHeader (:80-96) + where the data starts + loadPCD's field choice (:260-281) */
  fdm_pcd_field fields[FDM_PCD_MAX_FIELDS];
  int32_t n_fields;
  uint32_t width, height;       /* the cloud has width * height points (uint32 arithmetic); POINTS is ignored */
  uint32_t point_size;          /* bytes per binary record */
  double viewpoint[7];          /* tx ty tz qw qx qy qz; 0 0 0 1 0 0 0 unless VIEWPOINT has at least seven numbers */
  int32_t format;               /* FDM_PCD_ASCII (also: no DATA line, DATA without or with an unknown word) or FDM_PCD_BINARY */
  int32_t idx_x, idx_y, idx_z;  /* field indices, -1 = absent */
  int32_t idx_intensity;        /* the first of intensity, i, reflectivity */
  int32_t idx_rgb;              /* rgb, else rgba */
  int32_t idx_nx, idx_ny, idx_nz; /* normal_x / _y / _z, each falling back to nx / ny / nz; a channel only when all three exist */
  uint64_t data_offset;         /* the byte behind the DATA line's '\n' (n_bytes without one) */
} fdm_pcd_header;
/* parseHeader (:114-207) over the first n_bytes of a file; no byte behind them is read, no device is touched.  Lines
 * that are empty or start with '#' are skipped, tokens split on white space ('\r' included), keys and field names
 * compared lower-cased; SIZE / TYPE / COUNT lists shorter than FIELDS default to 4 / F / 1.  FDM_ERR_INVALID where the
 * reference throws or is undefined: no FIELDS, binary_compressed, WIDTH / HEIGHT without a number, a SIZE / COUNT /
 * WIDTH / HEIGHT / VIEWPOINT token std::stoul / std::stod rejects; and for more than 64 fields. */
int fdm_pcd_parse_header(const void* bytes, uint64_t n_bytes, fdm_pcd_header* header);
/* savePCD's header text (:454-488, :491 / :516) for a cloud of n points with these channels; viewpoint NULL = identity,
 * its numbers are printed with %g.  *n_bytes is the text's length (no NUL is written); FDM_SKIP_BUFFER_TOO_SMALL when
 * it exceeds cap (nothing is written).  No device is touched. */
int fdm_pcd_write_header(uint64_t n, int has_intensity, int has_rgb, int has_normal, const double* viewpoint, int format,
                         char* buf, uint64_t cap, uint64_t* n_bytes);
/* loadPCD's data section (:296-375): the records at `body` into caller-owned arrays of width * height entries, output
 * index == record index; any array may be NULL, and a channel the file lacks leaves its array untouched.  No point is
 * dropped: NaN and infinite values are loaded as they are.  rgb is the 4 bytes at the colour field, as 0x00RRGGBB.
 * Binary: each value goes through readFieldAsFloat (:209-230) — F4 (bits copied), F8 (rounded to nearest even), U1,
 * U4, I4; every other type / size pair reads as 0.0f — in the k_pcd_decode kernel; a pageable host body is copied to
 * the device once, a pinned one (fdm_host_alloc) is read in place when it starts on a 16-byte boundary (copied otherwise), a
 * device body may start at any byte.  ASCII: one
 * line per point, the value of a field is the token at the field's index (COUNT is not accounted for, as in the
 * reference), parsed on the host and uploaded when the outputs are device arrays.
 * FDM_ERR_INVALID: no x, y or z field; a body shorter than width * height * point_size or with too few lines or
 * tokens; a token std::stof / std::stoul rejects; and, for binary files, what the reference leaves undefined or this
 * library does not take: a point_size of 0, a chosen field (the colour field: its 4 bytes) reaching beyond the
 * record, a point_size above 1024.  Synchronous. */
int fdm_pcd_decode(const fdm_pcd_header* header, const void* body, uint64_t body_bytes, int body_on_device, float* x,
                   float* y, float* z, float* intensity, uint32_t* rgb, float* nx, float* ny, float* nz, int out_on_device,
                   int device);
/* savePCD's data section (:490-545) for n points into the host buffer `out`: fields x y z, then intensity, rgb
 * (r << 16 | g << 8 | b: the low 24 bits), normal_x normal_y normal_z, each present iff its array is given (the normals:
 * all three or none).  The arrays are host (on_device 0) or device arrays.  Binary records (12 to 32 bytes) are packed
 * by the k_pcd_pack kernel; ASCII lines are written on the host with std::fixed at `precision` (the reference's
 * default: 8), the colour as a decimal integer.  *n_bytes is the section's size; FDM_SKIP_BUFFER_TOO_SMALL when it
 * exceeds cap (nothing is written). */
int fdm_pcd_encode(uint64_t n, const float* x, const float* y, const float* z, const float* intensity, const uint32_t* rgb,
                   const float* nx, const float* ny, const float* nz, int on_device, int format, int precision, int device,
                   void* out, uint64_t cap, uint64_t* n_bytes);
/* buildDEM(loadPCD(file), cfg) (pcd2dem.cpp:38-44): the records are decoded into library-owned device arrays and take
 * the device path of fdm_engine_build_dem, with its statuses — FDM_SKIP_EMPTY_CLOUD for a file of 0 points, a file with
 * a coordinate that is not finite is refused by the outlier removal — and those of fdm_pcd_decode. */
int fdm_pcd_build_dem(const fdm_pcd_header* header, const void* body, uint64_t body_bytes, int body_on_device,
                      const fdm_dem_config* cfg, int device, fdm_engine** out_engine, fdm_dem_stats* stats);
/* The binary data section of savePCD(toPointCloud(map)) (pcd2dem.cpp:51-54) into the host buffer `out`:
 * fdm_engine_to_point_cloud_device, the pack kernel, one download.  Records are x y z [intensity] [rgb] as
 * *has_intensity / *has_color say; *n_bytes = *n_points * the record size; FDM_SKIP_BUFFER_TOO_SMALL when that exceeds
 * cap (nothing is written; rows * cols * 20 bytes always suffice). */
int fdm_engine_to_pcd(fdm_engine* e, void* out, uint64_t cap, uint64_t* n_bytes, uint64_t* n_points, int32_t* has_intensity,
                      int32_t* has_color);

/* Pinned host memory for input clouds (the arrays fdm_engine_integrate* read in place, see
 * fdm_engine_integrate_async).  Blocks come from a process-wide pool of hipHostMalloc'ed memory in
 * power-of-two size classes — a cloud allocated per sensor message costs a free-list pop, not a
 * driver call — and go back to the pool on fdm_host_free; fdm_host_trim() returns the pool's idle
 * blocks to the system.  Thread-safe.  Without a usable GPU the block is ordinary (pageable) memory,
 * which the engine then copies instead of reading in place; fdm_host_is_pinned tells which.
 * (Replaces the std::vector storage behind nanopcl::PointCloud, point_cloud.hpp:126-134.) */
void* fdm_host_alloc(uint64_t bytes);
void fdm_host_free(void* p);
void fdm_host_trim(void);
int fdm_host_is_pinned(const void* p);

/* Parity / measurement instrumentation (not in the reference). */
int fdm_engine_enable_cell_ids(fdm_engine* e, int on);
/* per input point of the last scan: linear cell id (col*rows+row), -1 cropped, -2 outside map */
int fdm_engine_last_cell_ids(fdm_engine* e, int32_t* host_out, uint64_t n);
int fdm_engine_enable_profile(fdm_engine* e, int on);
/* HIP-event durations of the last scan's launches: ms[0] = bin kernel, ms[1] = update kernel.
 * When the update was held back (see fdm_engine_integrate_device) ms[0] is the fused launch
 * (previous scan's update + this scan's bin) and ms[1] ~ 0. */
int fdm_engine_last_kernel_ms(fdm_engine* e, float* ms2);

/* Tuning knobs for A/B measurements (bench.py); unknown keys and values outside the accepted set are an error.  One line
 * per option, in the order of the engine's option table (csrc/fdm_engine_opts.inl; struct EngineOptions in
 * csrc/fdm_engine_host.hpp carries the measurements behind each default); tests/test_option_table.py keeps the two alike.
 *  the scan path
 *   "wave_merge" 0/1        : k_bin merges same-cell runs inside the wavefront before the atomics (default 1)
 *   "bin_variant" 0/1/4     : bin kernel by scan size (0, default), one point per thread (1), LDS-staged (4)
 *   "overlap" 0/1           : hold the update of a small scan back and fuse it with the next scan's bin launch (1)
 *   "zero_copy" n           : host entry points read PINNED input arrays of up to n points in place (default 2^30;
 *                             0 = always copy)
 *   "records" 0/1           : estimator state packed into per-cell records (1, default) or one array per layer (0)
 *   "dense" 0/1             : update sweep visits every tile (1) or only stamped tiles (0); default: 1 on maps of up to
 *                             4 M cells
 *   "move_clear_basic" 0/1  : GridMap::move()'s strips clear {elevation, elevation_min, elevation_max} only (default 0:
 *                             every layer); such an engine takes no batch launches
 *  the large-scan pipeline (per-tile record pools)
 *   "tiled" 0/1             : on / off (default 1)
 *   "tiled_min" n           : ... for scans from n points up (default 2048, on maps with enough tiles; a value set by hand
 *                             lifts the map-size condition)
 *  the batch pipeline (fdm_engine_integrate_device_batch)
 *   "batch" 0/1             : group small scans into batch launches (default 1)
 *   "batch_max" n           : scans per launch, 2 .. 32; default 0 = automatic: 32 with the quantile estimator or with
 *                             raycasting on, 16 with Kalman alone
 *   "batch_fuse" 0/1        : hold a batch's update back for the next batch's launch (default 1)
 *   "batch_crop" 0/1        : evaluate the next batch's crops one launch ahead (default 1)
 *   "batch_walk" -1/0/1     : the chain of moves walked one launch ahead (default -1 = for the quantile estimator only)
 *   "batch_ray" 0/1         : raycasting inside the batches (default 1; 0 = such scans leave one by one)
 *   "batch_ray_seg" 1/4/8/16: lanes per ray of its walk on memory-side atomics (default 4)
 *   "batch_ray_lds" 0/1     : its walk on LDS images (1, default) or always on memory-side atomics (0)
 *   "batch_ray_parts" n     : workgroups per quadrant and scan of the LDS walk (0 .. 64; default 0 = fill the chip)
 *  the raycasting stage
 *   "voxel_small" 0/1       : the voxel filter without a sort for small scans (default 1; fdm_raycast.hpp k_vs_*); 0 = every
 *                             scan through the stable radix sort
 *   "voxel_small_max" n     : ... for scans of up to n points (1 .. 2^20, default 65536)
 *   "voxel_any_order" 0/1   : which point represents a voxel in raycasting's voxel filter (VoxelMode::ANY) and in
 *                             fdm_engine_voxel_any: 0 = ties in point order (stable sort, default), 1 = the order libstdc++'s
 *                             std::sort leaves, so maps match a g++ build of the reference bit for bit (fdm_introsort.hpp).
 *                             While it is 1 the sort-free small-scan filter is not used, and batch calls with raycasting on
 *                             take the scan-by-scan path (batch launches without raycasting are unaffected).  A held-back
 *                             stage leaves before the value changes
 *   "ray_large_min" n       : raycasting of scans from n points up takes the large-scan path (default 196608): ray queue
 *                             ordered by (angular sector, length class)
 *   "ray_wedge" 0/1         : ... and walks it with the sector's minimum-height window in LDS (fdm_raywedge.hpp, default 1;
 *                             0 = one lane per ray on memory-side atomics)
 *   "ray_overlap" -1/0/1    : the stage's map-independent part (voxel filter, queue, walk) of a large scan leaves on a stream of its
 *                             own as soon as the scan's bin half has run, its resolve stays behind the scan's update (0, default:
 *                             never; 1 whenever possible; -1 for synchronous calls and scans of >= 1 M points).  Worth 10-14 % in a
 *                             process with few active streams, a loss in one with many
 *  measurement only (scripts/ab_kernels.py and the probes beside it; all default 0)
 *   "dbg_batch" n, "dbg_ray" n : bit switches of the batch and raycasting kernels
 *   "dbg_timeline" 0/1      : block start / end ticks of the fused large-scan launches (fdm_engine_debug_timeline) */
int fdm_engine_set_option(fdm_engine* e, const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* FDM_ENGINE_H */
