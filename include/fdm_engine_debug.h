/* fdm_engine_debug.h — measurement / debugging entry points of libfdm_engine.so.
 *
 * NOT part of the drop-in boundary (include/fdm_engine.h): nothing here corresponds to a call of the reference, a
 * host that replaces FastDEM::integrate never needs them.  They exist for bench.py (device-side stopwatch around a
 * batch call), the timeline / soak scripts under scripts/ and the tests that have to see which pipeline a call took. */
#ifndef FDM_ENGINE_DEBUG_H
#define FDM_ENGINE_DEBUG_H

#include "fdm_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdm_engine_integrate_device_batch between fdm_engine_timer_start and fdm_engine_timer_stop, i.e. the held-back
 * update of the last scan is launched and fdm_engine_timer_ms returns the device-side duration of the whole batch. */
int fdm_engine_integrate_device_batch_timed(fdm_engine* e, uint32_t count, const fdm_device_scan* scans);

/* After everything enqueued has run: how many entries of the small-scan batch pipeline's scratch sets are not in
 * their clean state (keys, aux words, zero-sign words) — 0 0 0 in a healthy engine. */
int fdm_engine_debug_batch_dirty(fdm_engine* e, uint64_t out[3]);

/* Engine option "dbg_timeline" = 1: start / end time of every block of the last fused large-scan launch (update of
 * scan t | bin of scan t + 1), in ticks of the 100 MHz constant clock — ticks[2*b], ticks[2*b + 1] for block b;
 * blocks [0, *n_update_blocks) are tile-update groups, the rest bin blocks.  Waits for the stream. */
int fdm_engine_debug_timeline(fdm_engine* e, uint64_t* ticks, uint64_t cap_blocks, uint32_t* n_blocks,
                              uint32_t* n_update_blocks);

/* How many batch launches the engine has enqueued since it was created: out[0] small-scan batches (k_mbatch,
 * fdm_multi.hpp), out[1] always 0 (the tile batches of round 4 are gone).  Tests assert with it that a call really took the
 * pipeline they mean to check. */
int fdm_engine_debug_batch_launches(fdm_engine* e, uint64_t out[2]);

/* Which kernel the last fdm_engine_apply_inpainting / _spatial_smoothing / _uncertainty_fusion / _feature_extraction call
 * launched, with its template arguments as the launch site spells them ("k_fusion_f64_tiled<29, true>", "k_median_sel"),
 * copied into out[cap] and always terminated; the empty string when the call returned before it launched (a disabled
 * fusion, a missing layer, zero inpainting passes).  Host bookkeeping only: nothing is read from the device. */
int fdm_engine_debug_last_post_kernel(fdm_engine* e, char* out, int cap);

/* fdm_pcd_debug_profile(1): the calling thread's PCD kernels are timed with device events from now on (off by
 * default; scripts/pcd_bench.py).  fdm_pcd_debug_last_kernel_ms: ms2[0] the k_pcd_decode launch of the last
 * fdm_pcd_decode / fdm_pcd_build_dem of a binary file, ms2[1] the k_pcd_pack launch of the last binary fdm_pcd_encode /
 * fdm_engine_to_pcd; copies are not included; zeros while the switch is off. */
int fdm_pcd_debug_profile(int on);
int fdm_pcd_debug_last_kernel_ms(float ms2[2]);

/* fdm_cloud_debug_profile(1): the calling thread's fdm_cloud_voxel_grid / fdm_cloud_grid_max_z calls are timed with
 * device events from now on (off by default: no event is created; scripts/voxel_bench.py).  fdm_cloud_debug_last_ms:
 * device ms of the last such call — keys and sort, run heads and staging, per-run reduction; zeros while the switch is
 * off.  The same switch times fdm_cloud_estimate_normals' stages (fdm_normal_stats.ms, fdm_engine.h). */
int fdm_cloud_debug_profile(int on);
int fdm_cloud_debug_last_ms(float ms3[3]);

/* fdm_segment_debug_batch(b): the calling thread's fdm_cloud_segment_plane / _planes calls score b hypotheses per launch
 * from now on (1 .. 128; 0 = the default again; scripts/segment_bench.py).  The result does not depend on it: the loop
 * is replayed in order whatever the batch (fdm_segment_stats.batch reports what a call used). */
int fdm_segment_debug_batch(int batch);

#ifdef __cplusplus
}
#endif
#endif
