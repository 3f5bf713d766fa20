// fdm_engine_host.hpp — what the translation units of libfdm_engine.so share: the engine object behind the C ABI and the
// host helpers one unit defines for the others.  The library is FIVE objects (one 2 000-line unit + 8 .inl + 13 kernel
// headers used to be one hipcc invocation, every A/B a full rebuild): fdm_engine.hip (the small-scan path: bin / update
// kernels, layers, options, the C entry points), fdm_engine_tiled.hip (the large-scan pipeline: record pools, k_tbin /
// k_tupdate), fdm_engine_multi.hip (the batch pipeline: k_mbatch, raycasting inside batches), fdm_engine_ray.hip (the
// raycasting stage of one scan: voxel filter, sorts, ray queue, walks, resolve), fdm_engine_post.hip (stencils, egress,
// ingest).  Non-template kernels in the shared headers are `inline` (weak symbols: one definition per library), a unit
// emits only the kernels it launches.
#pragma once
#include "../../include/fdm_engine.h"
#include "../../include/fdm_engine_debug.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>


#include "fdm_kernels.hpp"
#include "fdm_tiled.hpp"
#include "fdm_multi.hpp"
#include "fdm_route.hpp"
#include "fdm_raycast.hpp"
#include "fdm_introsort.hpp"
#include "fdm_voxel.hpp"
#include "fdm_raywedge.hpp"
#include "fdm_rbatch.hpp"
#include "fdm_rsort.hpp"
#include "fdm_egress.hpp"
#include "fdm_render.hpp"
#include "fdm_raster.hpp"
#include "fdm_knn.hpp"
#include "fdm_dem.hpp"
#include "fdm_pcd.hpp"
#include "fdm_ingest.hpp"
#include "fdm_post.hpp"
#include "fdm_normals.hpp"
#include "fdm_register.hpp"
#include "fdm_register_host.hpp"
#include "fdm_vgicp.hpp"
#include "fdm_segment.hpp"
#include "fdm_segment_host.hpp"
#include "fdm_cluster.hpp"
#include "fdm_cluster_host.hpp"

using namespace fdm;

// (the helpers every translation unit of the library shares: defined in fdm_engine.hip)
namespace fdmh {
int fail(int code, const std::string& msg);  // remembers the message for fdm_last_error(), returns `code`
}
using namespace fdmh;

#define HIPCK(expr)                                                                        \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return fail(FDM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)

namespace fdmh {
struct Layer {
  std::string name;
  float* d = nullptr;    // own array (stride 1), or nullptr when the layer is a record field
  int field = -1;        // index inside the cell record, -1 = own array
  bool pending = false;  // allocated, but not yet visible (lazy intensity / colour layers)
};
}  // namespace fdmh

namespace {
// field order inside the cell records (KalmanField / P2Field in fdm_kernels.hpp)
const char* const kKalmanFields[KF_COUNT] = {"elevation", "elevation_min", "elevation_max", "variance",
                                             "n_points", "_kalman_p", "_sample_mean", "_sample_m2",
                                             "upper_bound", "lower_bound"};
const char* const kP2Fields[PF_COUNT] = {"elevation", "elevation_min", "elevation_max", "variance",
                                         "n_points", "_p2_q0", "_p2_q1", "_p2_q2", "_p2_q3", "_p2_q4",
                                         "_p2_n0", "_p2_n1", "_p2_n2", "_p2_n3", "_p2_n4",
                                         "upper_bound", "lower_bound"};

const char* const kP2Q[5] = {"_p2_q0", "_p2_q1", "_p2_q2", "_p2_q3", "_p2_q4"};
const char* const kP2N[5] = {"_p2_n0", "_p2_n1", "_p2_n2", "_p2_n3", "_p2_n4"};
}  // namespace

// The values fdm_engine_set_option writes: one plain int each, one row of kOptions (fdm_engine_opts.inl) each, in the
// table's order.  The comment on a field is the option's documentation: what it selects and what was measured.  State
// DERIVED from an option (tiled_forced, Scratch::dense, the timeline buffer ...) stays in fdm_engine.
struct EngineOptions {
  // ---- the scan path ----
  int wave_merge = 1;               // option "wave_merge": k_bin merges same-cell runs inside the wavefront before the atomics
  int bin_variant = 0;  // 0 = by scan size, 4 = k_bin4 (LDS-staged), 1 = k_bin (one point/thread)
  int overlap = 1;                  // option "overlap": the update of a plain scan is held back and leaves with the next scan's bin half (enqueue_scan)
  // fdm_engine_integrate_async: scans of up to this many points whose arrays are PINNED host memory
  // are read in place by the bin kernel (0 = always stage with copy commands; option "zero_copy")
  int zero_copy = 1 << 30;
  int records = 1;                  // option "records": pack the active estimator's state into cell records (1, default) or one array per layer (0)
  int move_clear_basic = 0;         // option "move_clear_basic": GridMap::move()'s strips clear {elevation, elevation_min, elevation_max} only (the other reading of nanoGrid: DESIGN.md §6); such an engine takes no batch launches
  // ---- the large-scan (tiled) pipeline ----
  int tiled = 1;                    // option "tiled": large scans go through per-tile record pools
  int tiled_min = 2048;             // ... from this many points up (on a map of >= 512 tiles the pipeline wins at every
                                    // size measured: 2 K points 13.1 vs 14.6 us, 32 K 16.6 vs 20.5, 262 K 18.9 vs 34.3)
  // ---- the batch pipeline ----
  int batch = 1;                     // option "batch": fdm_engine_integrate_device_batch groups eligible scans
  int batch_max = 0;                 // option "batch_max": scans per launch (2 .. kMaxBatch = 32); 0 = automatic: 32 with the quantile
                                     // estimator or with raycasting on (configs[1] with it: 9.25 -> 7.78 us per scan), 16 with Kalman
                                     // alone — measured (profiles/r06/batch_max.txt): configs[2] (P2, 272 K-point
                                     // scans) 52.8 -> 56.9 G pts/s at 32, configs[1] (Kalman, 28.8 K-point scans) 27.0 -> 26.2: that
                                     // launch is within ~2 x of its instruction-issue floor, a second round of blocks only adds its time
  int batch_fuse = 1;                // option "batch_fuse": hold a batch's update back for the next batch's bin launch
  int batch_crop = 1;                // option "batch_crop": evaluate the next batch's crops one launch ahead
  int batch_walk = -1;               // option "batch_walk": the chain of moves walked one launch ahead (fdm_multi.hpp mwalk_body): -1 = for the quantile estimator only, 0 off, 1 on
  int batch_ray = 1;                 // option "batch_ray": 0 = an engine with raycasting on takes the single-scan path
  int batch_ray_seg = 4;             // option "batch_ray_seg": lanes per ray of k_rb_ray (1, 4, 8, 16)
  int batch_ray_lds = 1;             // option "batch_ray_lds": 0 = always the global-atomic walk (k_rb_ray)
  int batch_ray_parts = 0;           // option "batch_ray_parts": workgroups per quadrant and scan of k_rb_ray_lds (0 = fill the chip)
  // ---- the raycasting stage ----
  int voxel_small = 1;               // option "voxel_small": scans of <= 64 K points take the sort-free voxel filter
  int voxel_small_max = 1 << 16;     // option "voxel_small_max": largest scan that takes it
  // option "voxel_any_order": 0 = ties inside a voxel in point order (stable sort, default); 1 = the order libstdc++'s
  // std::sort leaves (fdm_introsort.hpp), so VoxelMode::ANY picks what a g++ build of the reference picks.  While it is
  // on, the sort-free small-scan filter is not used and batch calls with raycasting go scan by scan (multi_run)
  int voxel_any_order = 0;
  // scans from this many points up: bucketed ray queue, one lane per ray (option "ray_large_min").  Stage time, shared-
  // ray segments vs this path: 131 K points 0.48 vs 0.52 ms, 262 K 0.78 vs 0.57, 524 K 1.17 vs 0.67, RGB-D 272 K 0.23 vs 0.19
  int ray_large_min = 196608;
  // large scans: the walk keeps an angular sector's minimum-height image in LDS (option "ray_wedge", fdm_raywedge.hpp;
  // 0 = one lane per ray on memory-side atomics, k_ray<., 1>)
  int ray_wedge = 1;
  // two stages in flight (option "ray_overlap", fdm_engine_ray.inl): the map-independent part of a large scan's stage
  // (voxel filter, queue, walk) leaves on a stream of its own as soon as the scan's bin half has been launched, by scan
  // parity; k_ray_resolve stays behind the scan's update on the main stream
  int ray_overlap = 0;               // option "ray_overlap": 0 = off (default), 1 = whenever possible, -1 = for synchronous calls (whose update
                                     // then runs beside the stage's first part) and scans of >= 1 M points.  Measured in a process of its
                                     // own (scripts/ray_overlap_ab.py): configs[3] streamed 336 -> 290 us per scan, synchronous integrate()
                                     // 0.344 -> 0.311 ms, configs[2] synchronous 0.106 -> 0.092 ms; a STREAM of 272 K-point scans is bound
                                     // by the host's launches and pays for the events: 95 -> 125 us.  OFF by default because the gain
                                     // depends on the process: HIP maps streams onto four hardware queues, and in a process that has used
                                     // more than that (bench.py by the time of its large raycasting leg) the three streams of a stage
                                     // share queues and the events serialise them: 339 -> 365 us (profiles/r06/ray_overlap_ab.txt)
  // ---- measurement only ----
  int dbg_batch = 0;                 // measurement only (option "dbg_batch")
  int dbg_ray = 0;                   // option "dbg_ray": bit switches of the raycasting stage (RayParams::dbg)
};

// Everything ONE raycasting stage in flight writes, and what orders its uses (fdm_engine_ray.inl).  Every helper of the
// stage is told its bank and its stream; the engine has two banks (fdm_engine::ray_bank).
// WHO USES WHICH: bank 0 serves every stage that runs whole on the main stream (the normal path: run_held_ray_stage,
// fdm_engine_apply_raycasting*, fdm_engine_voxel_any) AND, with option "ray_overlap", the early part of even scans' stages
// on `stream`; bank 1 serves the early part of odd scans' stages only.  WHAT ORDERS THEM: a bank's next early part waits
// for `ev_res`, recorded on the main stream behind the last stage that used the bank — behind its k_ray_resolve on the
// early path, behind the whole stage on the normal path (bank 0, once the streams exist); the main stream waits for
// `ev_pre`, recorded behind an early part, before it resolves.  Buffers are allocated, grown and initialised on the MAIN
// stream (ensure_*), which may drain every stream; only a stage's launches (enqueue_*) go on the bank's stream.
struct RayBank {
  uint32_t* rc_cnt = nullptr;        // [ncell] ray-scan points observed in the cell this frame
  uint32_t* rc_min = nullptr;        // [ncell] ord(min ray height), kRayEmpty = not traversed
  uint32_t* ray_bins = nullptr;      // large scans: ray-queue bucket counts | offsets | block sums (fdm_raycast.hpp)
  unsigned long long* vkeys[2] = {nullptr, nullptr};  // voxel keys: unsorted / sorted
  uint32_t* vidx[2] = {nullptr, nullptr};             // point indices: unsorted / sorted
  uint32_t* vsel = nullptr;          // voxel_any output staging
  uint32_t* ray_blk = nullptr;       // rays queued per block of k_ray_compact (large scans: block-local queue regions)
  size_t vcap = 0;                   // points the voxel / queue buffers hold
  uint32_t* sort_tmp = nullptr;      // the radix sort's histograms (fdm_rsort.hpp: rs_hist_words(vcap))
  void* is_buf = nullptr;            // fdm_introsort.hpp's level buffers, rank tables, segment lists (is_layout)
  size_t is_cap = 0;                 // pairs is_buf is laid out for
  hipStream_t stream = nullptr;      // where the bank's early parts run (ensure_ray_streams)
  hipEvent_t ev_pre = nullptr;       // behind the last early part, on `stream`
  hipEvent_t ev_res = nullptr;       // behind the last stage that used the bank, on the main stream
  bool res_pending = false;          // ev_res has been recorded
  void release() {                   // (fdm_engine_destroy: nothing is in flight)
    for (void* p : {(void*)rc_cnt, (void*)rc_min, (void*)ray_bins, (void*)vkeys[0], (void*)vkeys[1], (void*)vidx[0],
                    (void*)vidx[1], (void*)vsel, (void*)ray_blk, (void*)sort_tmp, is_buf})
      if (p) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
    for (hipEvent_t ev : {ev_pre, ev_res})
      if (ev) (void)hipEventDestroy(ev);
  }
};

struct fdm_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  fdm_config cfg{};
  EngineOptions opt;               // what fdm_engine_set_option sets (above)
  GeomConst G{};
  size_t ncell = 0;
  std::vector<Layer> layers;
  float** d_layer_ptrs = nullptr;  // device array of every layer pointer (strip clears)
  int n_layer_ptrs = 0;
  bool layer_ptrs_dirty = true;
  Scratch S{};
  DevState* d_state = nullptr;
  DevState* h_state = nullptr;  // pinned mirror for read-backs
  StatsOut* h_stats = nullptr;  // pinned + device-mapped: k_collect_stats writes here
  StatsOut* h_stats_dev = nullptr;  // the device's alias of h_stats
  unsigned long long stats_seq = 0; // sequence number of the last statistics launch (StatsOut::seq)
  StatsAcc* d_stats_acc = nullptr;
  uint64_t scan_no = 0;
  bool have_scan = false;
  uint32_t last_n = 0;        // points of the last scan as enqueued (array length of the captures / cell ids)
  uint32_t last_n_input = 0;  // ... as the reference counts them (cloud.size(): finite points of a PointCloud2)
  int next_drop_nonfinite = 0;  // set by fdm_engine_integrate_cloud2 for the scan it enqueues
  unsigned ingest_blocks = 0; // > 0: the last scan came through k_ingest_soa; its finite count is still on the device
  int last_was_integrate = 0;
  // staging for the host-pointer entry points
  float* d_stage = nullptr;
  float4* d_aos = nullptr;  // fdm_engine_integrate_points4 on pageable memory: the cloud's {x, y, z, 1} records
  size_t aos_cap = 0;
  size_t stage_cap = 0;  // in points
  int stage_rr = 0;      // rotating staging block
  int32_t* d_cell_ids = nullptr;
  size_t ids_cap = 0;
  bool want_ids = false;
  bool profile = false;
  size_t bin_part_cap = 0;   // blocks
  unsigned last_bin_blocks = 0;
  std::vector<unsigned long long> h_bin_part;
  unsigned n_tiles = 0;
  std::vector<uint32_t> h_upd_part;
  bool obst_dense_pending = false;  // host wrote the obstacle layer / the pipeline changed: the next scan that observes a
                                    // cell clears it densely — which scan that is only the device knows (DevState::
                                    // dense_owed / dense_paid); the flag falls at the first sync behind it
  bool obst_owe_armed = false;      // ... the device has been told about the current debt
  unsigned obst_owe_seq = 0;
  bool estimator_ready = false;     // ElevationMapping ctor ran (ensureLayers + obstacle layer)
  float* d_rec = nullptr;           // [ncell][rec_floats]
  int rec_kind = -1;                // -1 none, 0 Kalman, 1 P2
  int rec_floats = 0;
  float* d_tmp = nullptr;           // ncell floats: contiguous staging for strided layer transfers
  bool cap_pre = false, cap_ras = false;  // scan-callback captures
  bool cap_cov = false;                   // ... the preprocessed cloud with its 3x3 covariance channel
  float* d_cap = nullptr;            // 4 channels x cap_cap points
  size_t cap_cap = 0;
  // the preprocessed cloud of a scan whose raycasting stage is HELD BACK with its update (enqueue_scan's ray_held): by scan
  // parity — the next scan's bin half writes its own while the stage of this one has not run yet; 3 channels x rcap_cap
  float* d_rcap[2] = {nullptr, nullptr};
  size_t rcap_cap = 0;
  float* d_ras = nullptr;            // ncell
  bool saved_want_ids = false;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float last_ms[3] = {0.f, 0.f, 0.f};
  // raycasting stage (fdm_raycast.hpp, host side: fdm_engine_ray.inl)
  RayBank ray_bank[2];               // the stage's buffers (above): [0] the normal path's, [k] the early stage's of scans of parity k
  hipEvent_t ev_ray_bin = nullptr;   // behind a scan's bin half on the main stream: that scan's early stage waits for it
  bool ray_bin_marked = false;       // ev_ray_bin was recorded behind the current scan's bin half (enqueue_scan)
  // the sort-free voxel filter of small scans (k_vs_*): normal-path stages on the main stream only, never an early stage
  uint32_t* vs_cnt = nullptr;        // fine | coarse bucket counters | valid points of k_vs_*
  uint4* vs_rec = nullptr;           // {key, point, bucket start, bucket size} by position
  size_t vs_rec_cap = 0;
  VoxelSmall vs{};                   // the last small-scan filter's parameters (k_vs_mark runs from enqueue_ray_walk)
  hipEvent_t ev_ray[2] = {nullptr, nullptr};
  hipEvent_t ev_timer[2] = {nullptr, nullptr};  // fdm_engine_timer_start / _stop
  bool ray_timed = false;
  bool sync_call = false;            // a synchronous entry point is running (its flush follows the enqueue at once)
  // update(t) || bin(t+1) in ONE launch (k_update_bin): the update of the last small scan is held back
  // until the next scan arrives (or any other entry point / sync flushes it); the scratch is
  // double-buffered by scan parity.
  unsigned long long* key2[2] = {nullptr, nullptr};  // scratch of even / odd scans ([0] == the original allocation)
  uint4* aux2[2] = {nullptr, nullptr};
  uint2* zs2[2] = {nullptr, nullptr};
  bool chain = false;           // an update is held back: the next bin derives its geometry from the previous slot
  struct BinVariant { bool bin4, has_int, has_col, wave_merge; unsigned threads; int lean; };  // lean: see bin4_body
  // the held-back update (plain data: the layer set cannot change while it is pending, every entry
  // point that could change it flushes first)
  struct PendingUpdate {
    bool multi = false;     // a whole batch (fdm_multi.hpp): MU / ch are what matters
    MUpd MU;
    int ch = 0;
    bool tiled = false;     // large-scan pipeline (fdm_tiled.hpp) or the per-cell scratch one
    ScanParams P;
    Scratch S;              // scratch pipeline: the key / aux set of the scan's parity, captures
    ScanInputs in;          // scratch pipeline: where the winning points are gathered from
    TilePool Q;             // tiled pipeline: the record pool of the scan's parity
    TileAux A;
    unsigned n_upd_blocks = 0;
    // the scan's raycasting stage (fastdem.cpp:152-159), which runs right behind this update wherever that is launched
    bool ray = false;
    int ray_pre = 0;        // 1 + bank if the stage's first part already left on that bank's stream (ray_overlap)
    RayParams RQ;
    const float *ray_x = nullptr, *ray_y = nullptr, *ray_z = nullptr;  // the scan's preprocessed cloud (d_rcap[parity])
    double ray_box[6] = {0, 0, 0, 0, 0, 0};
  } pend;
  // ---- tiled pipeline state (allocated when the first large scan arrives) ----
  bool tiled_forced = false;        // tiled_min was set by hand (option "tiled_min"): no map-size condition
  size_t tile_rare_waves = 0;       // update wavefronts the rare-path scratch is sized for
  TileGrid TG{};
  TilePool pool[2] = {};            // by scan parity
  size_t pool_cap = 0;              // records per pool
  unsigned desc_stride = 0;
  uint32_t* tile_stamp32 = nullptr;
  uint32_t* upd_part32 = nullptr;
  uint32_t* tile_rare = nullptr;    // the update's rare-path scratch, 3 KB per update wavefront
  unsigned last_upd_tiles = 0;      // length of the per-tile statistics of the last scan
  uint32_t* last_upd_part = nullptr;
  int last_kind = -1;               // pipeline of the last scan (0 scratch, 1 tiled)
  int last_do_move = 0, last_gate = 0;
  // ---- batch pipeline (fdm_multi.hpp): up to kMaxBatch small scans per launch, allocated by the first batch ----
  unsigned long long* mkey[2] = {nullptr, nullptr};  // [kMaxBatch][ncell] per batch parity
  uint4* maux[2] = {nullptr, nullptr};
  uint2* mzs[2] = {nullptr, nullptr};
  float2* mobs[2] = {nullptr, nullptr};              // [kMaxBatch][mobs_stride]
  uint32_t* mcobs[2] = {nullptr, nullptr};
  size_t mobs_stride = 0;
  unsigned long long* mbin_part[2] = {nullptr, nullptr};
  size_t mbin_cap = 0;
  uint32_t* mupd_part = nullptr;     // [update blocks] touched cells of a batch's last scan
  MState* mstate = nullptr;          // [kMStates] ring, slot = batch number % kMStates
  unsigned mseq = 0;                 // batches enqueued so far
  int last_batch_n = 0;              // scans of the batch launch the last scan left in (0: it took the single-scan path)
  uint64_t n_mbatch = 0;             // batch launches since creation (fdm_engine_debug_batch_launches)
  bool fault_watch = false;          // a launch that can raise DevState::fault was enqueued since it was last read (none can since round 4)
  unsigned long long batch_call = 0; // calls of fdm_engine_integrate_device_batch so far: a look-ahead is only ever honoured inside the call that made it
  unsigned long long pre_call = 0;
  bool pre_valid = false;            // the last launch carried the crop pass of the batch (pre_scans, pre_count) = number pre_seq
  const fdm_device_scan* pre_scans = nullptr;
  uint32_t pre_count = 0;
  unsigned pre_seq = 0;
  const unsigned long long* last_bin_part = nullptr;  // per-block statistics of the last scan (either pipeline)
  // ---- raycasting inside the small-scan batches (fdm_rbatch.hpp) ----
  unsigned rb_lds_words = 0;         // dynamic LDS k_rb_ray_lds may use, in 32-bit words (0: not asked yet)
  RState* rb_state = nullptr;
  float* rb_cap = nullptr;           // [3][kMaxBatch][rb_stride] preprocessed clouds of the batch being binned
  uint32_t* rb_u32 = nullptr;        // keys | place | sel | ray_list, [kMaxBatch][rb_stride] each
  uint4* rb_rec = nullptr;           // [kMaxBatch][rb_stride]
  uint32_t* rb_counters = nullptr;   // fine [kMaxBatch][2^18] | coarse [kMaxBatch][kVsCoarse]
  uint32_t* rb_img = nullptr;        // rc_cnt [kMaxBatch][ncell] | rc_min [kMaxBatch][ncell]
  size_t rb_stride = 0;
  unsigned rb_seq = 0;               // stamp of the last batch's ray launches (RState::any)
  float* d_bstage = nullptr;         // fdm_engine_integrate_host_batch: pageable clouds of a call, staged back to back
  size_t bstage_cap = 0;             // floats
  bool bstage_busy = false;          // launches of the previous call may still be reading it
  // scan routing (fdm_route.hpp)
  uint8_t* d_route_owner = nullptr;  // [route_cap] owner rank of every point of the slice
  uint32_t* d_route_cnt = nullptr;   // [route_blocks_cap][world + 2] block counts -> offsets | [kMaxRanks] bases at the end
  size_t route_cap = 0, route_blocks_cap = 0;
  // stencil post-processing (fdm_post.hpp)
  RegionEntry* d_region = nullptr;   // region_cap entries
  size_t region_cap = 0;
  float* d_post_pool = nullptr;      // per-thread lists of the big-neighbourhood stencil kernels
  size_t post_pool_cap = 0;          // in floats
  const char* last_post_kernel = ""; // kernel of the last stencil-stage call, as its launch site spells it ("": none was launched)
  FeatEntry* d_feat_tab = nullptr;   // kMaxRegion entries: the region as k_features_tiled reads it
  std::vector<RegionEntry> h_region; // what d_region holds (upload_region skips an identical table)
  std::vector<FeatEntry> h_feat_tab; // what d_feat_tab holds
  unsigned long long* d_timeline = nullptr;  // measurement only: {start, end} ticks per block of the last fused launch
  unsigned timeline_cap = 0;         // blocks the buffer holds
  unsigned timeline_blocks = 0, timeline_upd = 0;  // grid of the last fused launch, its update blocks
  unsigned timeline_bin = 0;         // ... its bin blocks (batch launches: the rest are crop blocks)
  float* d_tmp2 = nullptr;           // second ncell staging array (fusion works on two layers)
  // ingest (fdm_ingest.hpp)
  uint8_t* d_blob = nullptr;         // raw message bytes
  size_t blob_cap = 0;
  float* d_in = nullptr;             // 5 channels x in_cap: x y z intensity rgb
  size_t in_cap = 0;
  uint64_t in_n = 0;
  bool in_has_int = false, in_has_rgb = false;
  // egress (fdm_egress.hpp)
  uint32_t* pack_counts = nullptr;   // per-block valid counts / offsets (+1 for the total)
  size_t pack_counts_cap = 0;
  float* d_pack = nullptr;           // packed records
  size_t pack_cap = 0;               // in floats
  // layer images (fdm_render.hpp)
  uint32_t* d_image = nullptr;       // RGBA8 pixels of the last render, row-major
  size_t image_cap = 0;              // in pixels
  RenderState* d_render = nullptr;   // histograms, ranks, the normalisation range
  // static point clouds (fdm_raster.hpp, host side: fdm_engine_raster.inl); grown on demand, kept for the next call
  uint32_t* pc_keys[2] = {nullptr, nullptr};  // (cell id, point index) pairs: the two sides of the radix sort
  uint32_t* pc_idx[2] = {nullptr, nullptr};
  uint32_t* pc_hist = nullptr;       // the sort's histograms
  size_t pc_cap = 0;                 // points the pair buffers hold
  RasterStat* pc_stat = nullptr;     // counters / flags / bounding box the kernels leave
  float* pc_in = nullptr;            // fdm_engine_from_point_cloud: the host cloud's five channels, pc_in_cap points each
  size_t pc_in_cap = 0;
  float* pc_out = nullptr;           // toPointCloud's five channels, pc_out_cap points each
  size_t pc_out_cap = 0;
  uint32_t* pcd_rec = nullptr;       // fdm_engine_to_pcd's packed records, pcd_rec_cap words
  size_t pcd_rec_cap = 0;
  float pc_ms[3] = {0.f, 0.f, 0.f};  // ids / grouping / walk of the last fromPointCloud (profile on)
  hipEvent_t pc_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // ... and the events they are taken with (created on first use)
};

// ---- helpers shared by the library's translation units ----
namespace fdmh {
int join_streams(fdm_engine* e);  // (a null engine: FDM_OK — every C entry point starts with it, ahead of its null checks)
void poll_dense_paid(fdm_engine* e);
int sync_all(fdm_engine* e);
int pick_device(int device);  // the ordinal checked against the devices there are, then made current
struct ScopedDevice {  // the thread's current device, put back when an engine-free cloud call returns
  int prev = -1;
  ScopedDevice() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~ScopedDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
  ScopedDevice(const ScopedDevice&) = delete;
  ScopedDevice& operator=(const ScopedDevice&) = delete;
};
bool cloud_profile_on();  // fdm_cloud_debug_profile's switch for the calling thread (fdm_engine_voxel.inl)
// An engine-owned buffer that grows on demand: nothing if need <= *cap; else everything drains (sync_all), the old buffer
// is freed and forgotten (*ptr null, *cap 0: a failed allocation leaves an empty buffer, never a stale one), and `want`
// rows of `per` elements are allocated; *cap counts rows.  The contents are not kept.
int grow_device_bytes(fdm_engine* e, void** ptr, size_t* cap, size_t need, size_t want, size_t row_bytes);
template <typename T>
int grow_device(fdm_engine* e, T** ptr, size_t* cap, size_t need, size_t want, size_t per = 1) {
  return grow_device_bytes(e, reinterpret_cast<void**>(ptr), cap, need, want, per * sizeof(T));
}
Layer* find_layer(fdm_engine* e, const char* name);
float* lptr(fdm_engine* e, const Layer& l);
int lstride(fdm_engine* e, const Layer& l);
int fill_async(fdm_engine* e, float* p, float v, size_t n, int stride = 1);
int copy_strided(fdm_engine* e, float* dst, int ds, const float* src, int ss);
int ensure_tmp(fdm_engine* e);
int add_layer(fdm_engine* e, const char* name, float value, bool pending = false);
int ensure_layer(fdm_engine* e, const char* name, float value);
int refresh_layer_ptrs(fdm_engine* e);
int resolve_pending(fdm_engine* e);
float* L(fdm_engine* e, const char* n);
float* Lany(fdm_engine* e, const char* n, int* stride);
void fill_integrate_params(fdm_engine* e, ScanParams& P, const double* Tbs, const double* Twb);
int enqueue_scan(fdm_engine* e, ScanParams& P, uint64_t n, const ScanInputs& in, const ScanInputs* gather = nullptr,
                 bool in_engine_slot = false);
int read_stats(fdm_engine* e, fdm_scan_stats* out, int* status);
const void* pinned_alias(const void* p);
constexpr int kStageSlots = 3;  // rotating staging slots (see next_stage_slot)
// One slot of the engine's staging block: six channels of `cap` points each, in the order x, y, z, intensity, rgb,
// variance, at base + cap * 0..5 (cap is a multiple of 4 points: every channel starts 16-byte aligned).
struct StageSlot {
  float* base = nullptr;
  size_t cap = 0;
  float* x() const { return base; }
  float* y() const { return base + cap; }
  float* z() const { return base + cap * 2; }
  float* intensity() const { return base + cap * 3; }
  uint32_t* rgb() const { return reinterpret_cast<uint32_t*>(base + cap * 4); }
  float* var() const { return base + cap * 5; }
  // the slot as a scan's channels: x, y, z and those of the optional ones that it holds
  ScanInputs as_inputs(bool has_intensity, bool has_rgb, bool has_var) const {
    return {x(), y(), z(), has_intensity ? intensity() : nullptr, has_rgb ? rgb() : nullptr, has_var ? var() : nullptr};
  }
  // ... as the target of the bin kernel's write-through, which the held-back update gathers from: it never takes intensity
  ScanInputs as_gather() const { return as_inputs(false, true, true); }
};
int next_stage_slot(fdm_engine* e, size_t n, StageSlot* s);
int upload_channels(fdm_engine* e, uint64_t n, const ScanInputs& host, const StageSlot& s);
int stage_inputs(fdm_engine* e, uint64_t n, const ScanInputs& host, ScanInputs* dev, ScanInputs* gather = nullptr);
// the raycasting stage (fdm_engine_ray.hip), called from the scan path
bool voxel_size_ok(float v);
int ensure_ray_layers(fdm_engine* e);
VoxelCompact voxel_compact_of(float voxel_size, const double* box);
void ray_box_of(const fdm_engine* e, const ScanParams& P, double box[6]);
fdm_raycast_config ray_config_of(const fdm_config& c);
RayParams make_ray_params(fdm_engine* e, const fdm_raycast_config& c, const float* origin, unsigned n,
                          int slot, int flag_slot);
int run_held_ray_stage(fdm_engine* e, fdm_engine::PendingUpdate& u);
int start_ray_stage_early(fdm_engine* e, fdm_engine::PendingUpdate& u, const ScanParams& P);
// the large-scan pipeline (fdm_engine_tiled.hip)
int ensure_tile_aux(fdm_engine* e);
int ensure_tile_pool(fdm_engine* e, size_t records, unsigned blocks);
unsigned update_blocks(const fdm_engine* e, bool fused);
int launch_tbin(fdm_engine* e, const ScanParams& P, const ScanInputs& in, const TilePool& Q, int32_t* ids,
                unsigned bin_blocks, fdm_engine::BinVariant bv);
int launch_tiled_update_alone(fdm_engine* e, const fdm_engine::PendingUpdate& u);
int launch_tiled_update_fused(fdm_engine* e, const fdm_engine::PendingUpdate& u, const ScanParams& Pb,
                              const ScanInputs& Ib, const TilePool& Qb, int32_t* ids_b, unsigned bin_blocks_b,
                              fdm_engine::BinVariant bv);
// the batch pipeline (fdm_engine_multi.hip)
uint32_t multi_run(fdm_engine* e, uint32_t count, const fdm_device_scan* scans);
int enqueue_multi(fdm_engine* e, uint32_t count, const fdm_device_scan* scans, uint32_t next_count);
int launch_multi_update(fdm_engine* e, const fdm_engine::PendingUpdate& u);
int launch_update_alone(fdm_engine* e, const fdm_engine::PendingUpdate& u);
P2Params p2_params(const fdm_config& c);
void sensor_params(const fdm_config& cfg, int& type, float* sp);
int ensure_estimator_layers(fdm_engine* e);
int ensure_scratch_channels(fdm_engine* e, bool intensity, bool color);
void rotation_of_product(const double* Twb, const double* Tbs, float* R);

// f(policy tag, layer set) for the engine's estimator and layer layout
template <typename F>
int with_policy(fdm_engine* e, F&& f) {
  const bool p2mode = e->cfg.estimation_type == 1;
  if (e->rec_kind >= 0) {  // cell records
    if (p2mode) {
      P2RecLayers Lr{};
      Lr.rec = e->d_rec; Lr.obstacle = L(e, "obstacle"); Lr.color = L(e, "color");
      Lr.intensity = Lany(e, "intensity", &Lr.istride);
      Lr.p = p2_params(e->cfg);
      return f(P2RecPolicy{}, Lr);
    }
    KalmanRecLayers Lr{};
    Lr.rec = e->d_rec; Lr.obstacle = L(e, "obstacle"); Lr.color = L(e, "color");
    Lr.intensity = Lany(e, "intensity", &Lr.istride);
    Lr.min_var = e->cfg.kalman_min_variance; Lr.max_var = e->cfg.kalman_max_variance;
    Lr.q = e->cfg.kalman_process_noise;
    return f(KalmanRecPolicy{}, Lr);
  }
  if (p2mode) {
    P2Layers Lp{};
    Lp.elevation = L(e, "elevation");
    Lp.elevation_min = L(e, "elevation_min");
    Lp.elevation_max = L(e, "elevation_max");
    Lp.variance = L(e, "variance");
    Lp.n_points = L(e, "n_points");
    Lp.upper = L(e, "upper_bound");
    Lp.lower = L(e, "lower_bound");
    Lp.obstacle = L(e, "obstacle");
    Lp.intensity = L(e, "intensity");
    Lp.color = L(e, "color");
    for (int k = 0; k < 5; ++k) {
      Lp.q[k] = L(e, kP2Q[k]);
      Lp.n[k] = L(e, kP2N[k]);
    }
    Lp.p = p2_params(e->cfg);
    return f(P2Policy{}, Lp);
  }
  KalmanLayers Lk{};
  Lk.elevation = L(e, "elevation");
  Lk.elevation_min = L(e, "elevation_min");
  Lk.elevation_max = L(e, "elevation_max");
  Lk.variance = L(e, "variance");
  Lk.n_points = L(e, "n_points");
  Lk.kalman_p = L(e, "_kalman_p");
  Lk.sample_mean = L(e, "_sample_mean");
  Lk.sample_m2 = L(e, "_sample_m2");
  Lk.upper = L(e, "upper_bound");
  Lk.lower = L(e, "lower_bound");
  Lk.obstacle = L(e, "obstacle");
  Lk.intensity = L(e, "intensity");
  Lk.color = L(e, "color");
  Lk.min_var = e->cfg.kalman_min_variance;
  Lk.max_var = e->cfg.kalman_max_variance;
  Lk.q = e->cfg.kalman_process_noise;
  return f(KalmanPolicy{}, Lk);
}
template <typename POLICY>
constexpr bool is_rec_policy = std::is_same<POLICY, KalmanRecPolicy>::value || std::is_same<POLICY, P2RecPolicy>::value;

// Runtime flags -> template arguments: with_constants(f, a, b, ...) calls f(A{}, B{}, ...), one std::integral_constant per
// argument — a bool as it is, UpTo<N>{v} as an int in 0 .. N - 1 (clamped).  Every launch site that picks a kernel variant
// by (has_int, has_col[, lean]) goes through it; f instantiates the whole product of its arguments, so a site whose
// kernels cover only part of it says so with `if constexpr`.
template <int N>
struct UpTo { int v; };
template <typename F>
auto with_constants(F&& f) { return f(); }
template <typename F, int N, typename... Rest>
auto with_constants(F&& f, UpTo<N> k, Rest... rest);
template <typename F, typename... Rest>
auto with_constants(F&& f, bool b, Rest... rest) {
  return b ? with_constants([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
           : with_constants([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}
template <typename F, int N, typename... Rest>
auto with_constants(F&& f, UpTo<N> k, Rest... rest) {
  if constexpr (N > 1) {
    if (k.v < N - 1) return with_constants(f, UpTo<N - 1>{k.v}, rest...);
  }
  return with_constants([&](auto... c) { return f(std::integral_constant<int, N - 1>{}, c...); }, rest...);
}

// kernels with more than 64 KB of dynamic LDS need the attribute once
template <typename K>
int allow_lds(K kern, unsigned bytes) {
  static std::mutex mu;
  static std::unordered_map<const void*, unsigned> seen;
  if (bytes <= 65536u) return FDM_OK;
  const void* f = reinterpret_cast<const void*>(kern);
  std::lock_guard<std::mutex> lock(mu);
  auto it = seen.find(f);
  if (it != seen.end() && it->second >= bytes) return FDM_OK;
  HIPCK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)));
  seen[f] = bytes;
  return FDM_OK;
}

}  // namespace fdmh
