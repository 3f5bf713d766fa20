// fdm_multi.hpp — a BATCH of small scans in ONE launch instead of one launch per scan.
//
// Why: a VLP-16 scan (28.8 K points, 113 bin blocks, 88 update blocks) is launch- and
// latency-bound: one fused launch per scan costs ~6 us — ~3 us of it the queue's own per-kernel floor, the rest
// two or three dependent memory round trips of ~3 us each under load.  fdm_engine_integrate_device_batch sees its
// scans up front, so up to kMaxBatch of them are binned by one launch into per-scan scratch sets and every cell
// thread of the update applies the batch's observations in scan order.  Per cell the reference only fixes the
// order of the scans (elevation_mapping.cpp:94-125: one independent update per observed cell and scan;
// GridMap::move strips and the obstacle-layer clear happen between scans), and that order is kept exactly — the
// map after the batch is bit-identical to integrating the scans one by one.
//
// One launch per batch, k_mbatch = [ update of batch b-1 | bin of batch b | scouts (+ walker) of batch b+1 ]:
//
//   scout rows   Scan k is binned against the map geometry AFTER the LOCAL-mode moves of scans 0..k, and whether
//                scan j moved the map depends on whether any of its points survived the crops (fastdem.cpp:138) —
//                device-side data.  The crops need no geometry, so the question is answered ONE LAUNCH AHEAD: a few
//                scout blocks per scan of the next batch (first transform + cropRange + cropZ, the same float
//                operations the bin half will run; first survivor, early exit) OR "scan k has a surviving point"
//                into the next batch's state word; the kernel boundary is the barrier.  The first batch of a call has
//                no launch ahead of it: its scouts run as a small launch of their own.  (Rounds 3: an in-launch protocol
//                for that case — every block adds itself to its scan's counter, later scans' blocks poll a state word,
//                bounded spin, a sticky fault when it ran out.  Gone: no block of this kernel ever waits for another.)
//                One more block of these rows, the WALKER (mwalk_body), walks the next batch's chain of moves ahead of
//                its launch, assuming every scan passes (on for the quantile estimator: option "batch_walk").
//   bin half     512 points per block (two per thread), scan k of the batch; the first wavefront walks the chain of k
//                moves (every lane rounds its own scan's pose once; only the position is accumulated in scan order;
//                the reference's divide only for poses on a rounding tie) while the point loads are in flight.
//                Points fold straight into a per-block LDS cell table (axis_fast indexing): both points of a thread
//                probe it in one batch, and the lane that finds a slot empty has CLAIMED it and numbers the cell's
//                record there (a ballot and one LDS add per wavefront) — so behind the fold's one barrier the records
//                are listed already, and they are flushed with memory-side atomics on the block's unique cells.
//                No second look at the scan: the thread that merges a block-local minimum into the scratch also
//                evaluates that point's sigma_z^2 (the block keeps its points' sensor-frame coordinates in LDS) and
//                stores {map-frame z, sigma_z^2} in an observation array at the block's SLOT for the cell (lb * kMBlock
//                + the record's number: a block's winners are one contiguous run); likewise the colour of a
//                block-local last point.  The order of the slots BETWEEN blocks is the order of the points ("the first
//                point wins", "the last colour wins"); the order inside a block is the order of the claims, depends on
//                timing and shows in no output.  The update finds the winner's entry through the slot in the
//                reduced key (aux.w for the colour), and the caller's arrays are dead as soon as the launch has run.
//   update half  64 cells per block (memory order), four threads per cell, laid out group-major: thread q * 64 + c looks
//                after scans 4 q .. 4 q + 3 of cell c, so wavefront q holds one group of four scans of all 64 cells and
//                a key load is one contiguous run of keys per scan.  Round trip 1: the cell's keys of all scans, its
//                estimator record, the per-scan geometry.  The cell's scan mask is OR-ed through a small LDS table
//                (its threads sit in different wavefronts).  The block's (cell, scan) events are then compacted into an
//                LDS list (kEvCap entries) and spread evenly over the threads: round trip 2 fetches {aux, zs, obs} of
//                ALL events at once (a thread holds 2-3 of them whatever their distribution over the cells), the
//                observations go back through LDS to the cell's OWNER — thread c, so the owners are wavefront 0, every
//                lane of it a cell, and wavefronts 1-3 skip the serial part — which walks its events in scan order:
//                strips vacated since the previous event, estimator step in registers, one record store.  (Beyond 16
//                scans: 32 cells per block, eight threads per cell, thread q * 32 + c, the owners lanes 0-31 of
//                wavefront 0.)  In the code: mupdate_body is the front all instantiations share (round trip 1, the
//                masks, the event numbers: mupd_commit, mupd_vacated, mupd_number), then the owners' walk of its
//                variant, which runs the rounds of the exchange (mupd_exchange) — mupd_walk_plain, or with
//                raycast_enabled (template RAY) mupd_walk_ray, which also
//                resolves every scan's raycasting stage behind that scan's observation — the images come from the
//                launches of fdm_rbatch.hpp between the launch that binned the batch and this one.
//   the chain    of moves has one arithmetic (lane_f64, mchain_nearest, mchain_shift), used by the walker (mwalk_batch)
//                and by the bin blocks' own walk (mbin_body).
//
// All per-batch parameters travel as kernel arguments (7.2 KB with 32 scans per batch; the limit kept is 8 KB,
// launch_mbatch's static_assert): no copy command, no upload kernel.  They are laid out by WHO reads them FIRST: a block
// waits for one scalar round trip (the head, see k_mbatch) and a bin or scout block for a second (its scan's record,
// MBinScan / MCropScan) before its vector loads leave.
// Algorithmic bytes are per scan what they were: 12 B/point (+4 intensity, +4 colour), 72 / 124 B per
// touched cell, 4 B per map cell per scan for the obstacle clear.
#pragma once

#include "fdm_kernels.hpp"

namespace fdm {

constexpr int kMaxBatch = 32;            // scans per launch (one bit per scan in 32-bit state words).  Round 6: 16 -> 32 — a
                                         // 16-scan VLP-16 batch is LESS than one round of blocks on the chip and pays the launch's
                                         // fixed costs (3.4 us queue floor, the first round trip of 1 264 blocks at once) in full
constexpr int kScansPerThread = 4;   // update half: a thread looks after four scans of its cell, so a cell takes four threads in
                                     // a batch of up to 16 scans (64 cells per block) and eight beyond (32 cells per block):
                                     // MUpd::tpc — at most 1 024 (cell, scan) events per block = two rounds of the exchange either way
// the n lowest bits (n <= 32: a shift by 32 is not a shift)
__host__ __device__ constexpr unsigned lowbits(unsigned n) { return n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u; }
constexpr int kLineWords = 32;           // a 128-byte line of 32-bit words
// "These values are in scalar registers HERE, all of them" (an input of an empty asm: a pointer that came OUT of one would
// be a pointer of unknown kind — flat loads, which count on both wait counters): no instruction, but the compiler can no longer sink the
// loads of kernel arguments that produce them behind a branch or behind each other's waits — loads that do not depend on
// one another leave as one batch and the wavefront waits for them once (k_mbatch's head, a scan's record).
// The other direction: a struct of the kernel arguments as seen from HERE on.  The compiler may not hoist a load of one of
// its members above this point — into the block that dispatches the halves, where it would be one more round trip in
// front of every block's first vector loads — and still knows the members are uniform constants (scalar loads): the
// struct's address gains an offset the compiler cannot see is zero, nothing escapes.
template <typename T>
__device__ __forceinline__ const T& kernarg_from_here(const T& v) {
  unsigned zero = 0u;
  asm volatile("" : "+s"(zero));
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(&v) + zero);
}
#define FDM_SGPR_NOW4(a, b, c, d) asm volatile("" ::"s"(a), "s"(b), "s"(c), "s"(d))
#define FDM_SGPR_NOW10(a, b, c, d, e, f, g, h, i, j) \
  asm volatile("" ::"s"(a), "s"(b), "s"(c), "s"(d), "s"(e), "s"(f), "s"(g), "s"(h), "s"(i), "s"(j))
#define FDM_SGPR_NOW11(a, b, c, d, e, f, g, h, i, j, k) \
  asm volatile("" ::"s"(a), "s"(b), "s"(c), "s"(d), "s"(e), "s"(f), "s"(g), "s"(h), "s"(i), "s"(j), "s"(k))
#ifndef FDM_MB_WAVES
#define FDM_MB_WAVES 6  // waves per SIMD k_mbatch is compiled for (<= 80 VGPRs; the LDS allows 6 blocks per CU): every block of a 16-scan VLP-16 batch resident at once
#endif
#ifndef FDM_KALMAN_WALK_FROM
#define FDM_KALMAN_WALK_FROM 0
#endif
constexpr int kKalmanWalkFrom = FDM_KALMAN_WALK_FROM;  // Kalman batches: the first scan whose bin blocks take the walker's chain (fdm_engine_multi.inl; 12 until profiles/r19/flush)
constexpr int kMStates = 4;              // ring of batch states: update b-1 | bin b | crop b+1 | being re-armed

// Device-resident bookkeeping of one batch.  Every word other blocks poll or add to sits on its own 128-byte
// line: pollers of `flags` must not queue up in front of the adds to `done`.
struct MState {
  DevGeom E[kMaxBatch];        // geometry before scan k (written by the scan's first bin block)
  DevCand C[kMaxBatch];        // geometry after its move + the index shift
  unsigned flags[kLineWords];  // [0]: bit k = scan k has a surviving point (scouts); [1]: the pass bits PE / PC below assume; [2]: != 0 = PE / PC are valid
  unsigned inside[kMaxBatch];  // some point of scan k landed in the map (elevation_mapping.cpp:118)
  unsigned pad[16];
  DevGeom PE[kMaxBatch];       // the chain of moves walked ONE LAUNCH AHEAD by the walker block (mwalk_body): geometry before
  DevCand PC[kMaxBatch];       // scan k / after its move, assuming the pass bits in flags[1]
};

struct MCommon {  // what all scans of a batch share
  float min_sq, max_sq, z_min, z_max;
  float sp[4];
  float Tbs[16];  // T_base_sensor (one sensor per batch: a scan with another extrinsic closes the batch)
  int sensor_type, integrate_mode, do_move, gate_on_filter, has_var;
  int pad0;  // (no kernel reads it.  It keeps the words behind it in the groups k_mbatch's scalar loads fetch them in: without it
             //  every instantiation is allocated differently and configs[1] measured 2.4 % slower, profiles/r14/retire)
  int dbg, walk;                 // walk: 1 = the chain of moves is walked one launch ahead (mwalk_body).  dbg, measurement only: 1 = no scratch atomics, 2 = no chain walk (both: wrong results); 3 = every move by the reference's divide (tests)
  int walk_from, pad;            // with walk: scans k >= walk_from take the pre-walked chain, the bin blocks of earlier scans walk their own
  unsigned long long* timeline;  // measurement only (nullable): {start, end} of every block in 100 MHz ticks
};
struct MScanT {   // per scan: T_world_base without its constant last row (0 0 0 1), column-major 3 x 4 | rotation of the product
  float Twb[12], R[9];
};
// One scan of the bin half.  A bin block knows its scan from the grid, and everything it needs of that scan before its
// point loads can leave — the pointers and n — sits on one 64-byte line of the arguments, the transforms behind it: one
// batch of scalar loads, one wait (parallel arrays n[], px[], py[] ... 256 bytes apart were a chain of dependent trips).
struct MBinScan {
  const float* px;
  const float* py;
  const float* pz;
  const float* pint;
  const uint32_t* prgb;
  const float* pvar;
  unsigned n, first_block;               // points of the scan | bin blocks before it
  MScanT t;
  unsigned pad;
};
struct MBin {     // bin half: batch b
  unsigned count, scan_no0;
  MState* ms;
  // The previous batch's state while its update shares this launch.  Always readable: with no previous batch it is the
  // batch's own state and has_prev is 0 (prev_count 1), so the loads through it leave unconditionally beside the
  // geometry ring's and the choice is a select on the values (mbatch_start, mbin_body)
  const MState* prev;
  unsigned prev_count, has_prev;
  unsigned obs_stride;                   // points per scan slot of obs / cobs
  unsigned pad;
  // per-scan scratch, slot k at + k * ncell (key, aux, zs as in Scratch)
  unsigned long long* key;
  uint4* aux;
  uint2* zs;
  float2* obs;                           // [count][obs_stride] {map-frame z, sigma_z^2} of block-local minima, by slot (mbin_body's merge)
  uint32_t* cobs;                        // [count][obs_stride] colour of block-local last points, by slot
  unsigned long long* bin_part;          // [bin blocks]
  float* cap;                            // raycasting: [3][count][obs_stride] map-frame x (NaN: dropped by the crops), y, z by point index (else null)
  double robot_x[kMaxBatch], robot_y[kMaxBatch];  // T_world_base translation of every scan (the chain of moves; read by lane)
  MBinScan s[kMaxBatch];
};
// Raycasting stage of the batch's scans (fastdem.cpp:152-159, once per scan BEHIND that scan's map update).  The ray
// launches of fdm_rbatch.hpp leave, per scan, the two order-free images of processScan — observed-evidence counts and the
// minimum ray height per cell — and the update half resolves them cell by cell, each scan's behind that scan's
// observation (resolveGhostCells, raycasting.cpp:175-202).
struct RState {   // device bookkeeping of a batch's ray launches (one per engine: they run between the launch that bins the batch and the one that updates it)
  unsigned any[kMaxBatch];        // == the batch's stamp: the voxel-filtered scan k is not empty (raycasting.cpp:207-209)
  unsigned origin_in[kMaxBatch];  // the sensor origin lies in the map after scan k's move (raycasting.cpp:217-220)
  unsigned qcount[kMaxBatch][4];  // queued downward rays of scan k, by the quadrant they leave the sensor's cell into
  unsigned total[kMaxBatch];      // valid points of scan k (VoxelSmall::total)
};
struct MRay {
  const RState* rs;
  unsigned stamp;          // 0: no raycasting in this batch
  unsigned pad;
  uint32_t* rc_cnt;        // [count][ncell] observed-evidence counts; zero between batches
  uint32_t* rc_min;        // [count][ncell] ord(min ray height); kRayEmpty between batches
  float* logodds;          // _visibility_logodds
  float* ray_min;          // raycasting
  float* ghost;            // ghost_removal
  float l_obs, l_ghost, l_max, clear_thr, conflict_thr;
  float pad2;
};
struct MUpd {     // update half: batch b-1 (the kernel's first struct argument: key and ms, which an update block's first
                  // loads go through, lie directly behind the head's scalars and are fetched with them)
  unsigned long long* key;
  MState* ms;
  unsigned count, scan_no0, obs_stride;
  int do_move, gate_on_filter;
  unsigned pad;
  MRay ray;
  MState* rearm;                         // the state of the batch after next: zeroed by the committing block
  uint4* aux;
  uint2* zs;
  const float2* obs;
  const uint32_t* cobs;
  uint32_t* upd_part;                    // [update blocks] cells touched by the batch's LAST scan
};
struct MCropScan {  // one scouted scan, as MBinScan: one batch of scalar loads
  const float* px;
  const float* py;
  const float* pz;
  unsigned n, pad;
};
struct MCrop {    // crop half: batch b+1 (count == 0: none)
  unsigned count, pad;
  MState* ms;
  // the walker block: the scouted batch's poses, and — when no batch is binned by this launch (the scout-only launch in
  // front of a call's first batch) — where its chain starts: the previous batch's state (complete), or the geometry ring
  // (has_prev 0: prev is then the scouted batch's own state, readable and unused, as MBin::prev)
  const MState* prev;
  unsigned prev_count, has_prev, scan_no0, pad1;
  double robot_x[kMaxBatch], robot_y[kMaxBatch];
  MCropScan s[kMaxBatch];
};

// The members the arithmetic reads, by name (pointers only: an array member copied in device code is spilled,
// see DevObst).
struct MView {
  const float* Tbs;
  const float* Twb12;
  const float* R;
  const float* sp;
  float min_sq, max_sq, z_min, z_max;
  int sensor_type, integrate_mode;
};
// the batch's shared members + one scan's transforms (null for the scouts: the crops need neither)
__device__ __forceinline__ MView mview(const MCommon& K, const float* Twb12, const float* R) {
  MView V;
  V.Tbs = K.Tbs; V.Twb12 = Twb12; V.R = R; V.sp = K.sp;
  V.min_sq = K.min_sq; V.max_sq = K.max_sq; V.z_min = K.z_min; V.z_max = K.z_max;
  V.sensor_type = K.sensor_type; V.integrate_mode = K.integrate_mode;
  return V;
}

// p <- T * p for a T whose last row is (0 0 0 1), stored without it: the same products and sums, in the same
// order, as transform4 on the full matrix (the row's coefficients are the literals 0 and 1).
__device__ __forceinline__ void transform4_affine(const float* __restrict__ t12, float& x, float& y, float& z, float& w) {
  float o[4];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float acc = t12[0 + r] * x;
    acc = t12[3 + r] * y + acc;
    acc = t12[6 + r] * z + acc;
    acc = t12[9 + r] * w + acc;
    o[r] = acc;
  }
  {
    float acc = 0.0f * x;
    acc = 0.0f * y + acc;
    acc = 0.0f * z + acc;
    acc = 1.0f * w + acc;
    o[3] = acc;
  }
  x = o[0]; y = o[1]; z = o[2]; w = o[3];
}
// first half of preprocess_point (T_base_sensor, cropRange, cropZ): does the point survive?  w rides along.
__device__ __forceinline__ bool mcrops(const MView& V, float& x, float& y, float& z, float& w) {
  w = 1.0f;
  transform4(V.Tbs, x, y, z, w);
  const float d2 = sum3(x * x, y * y, z * z);
  bool pass = (d2 >= V.min_sq) && (d2 <= V.max_sq);
  pass = pass && (z >= V.z_min) && (z <= V.z_max);
  return pass;
}

// LDS of one block: the bin half's cell table + point staging, or the update half's event exchange.
constexpr int kEvCap = 512;  // (cell, scan) events of a 256-cell tile exchanged per round (two per thread)
#ifndef FDM_M_PTS
#define FDM_M_PTS 2
#endif
constexpr int kMPts = FDM_M_PTS;                 // points per thread of the bin half: 512-point blocks — half the blocks (every block
constexpr unsigned kMBlock = 256u * kMPts;  // of a 16-scan batch resident beside the update half) and ~20 % fewer (block, cell) pairs
struct MBinLds {
  unsigned long long t_key[kMBlock];
  uint32_t t_cell[kMBlock], t_zmx[kMBlock], t_imx[kMBlock], t_fst[kMBlock], t_lst[kMBlock];
  float4 s_pt[kMBlock];  // sensor-frame x, y, z | map-frame z of the block's points
  uint16_t s_list[kMBlock];  // the table slots of the block's records, in the order they were claimed
  DevCand s_cand;
  unsigned s_pass[4], s_in[4];
  unsigned s_nrec;  // records so far: a wavefront adds its claims (mbin_body's fold)
};
struct MEvent { uint32_t idx; uint16_t cell, k; };  // winner's slot in obs | cell in tile | scan
struct alignas(16) MObs { float min_z, var, max_z, iobs; };  // (one 128-bit LDS access)
constexpr unsigned kUpdCells = 64u;   // cells per update block at most (MUpd::tpc == 4; 32 with eight threads per cell)
__host__ __device__ constexpr unsigned upd_threads_per_cell(unsigned count) { return count > 16u ? 8u : 4u; }
__host__ __device__ constexpr unsigned upd_cells_per_block(unsigned count) { return 256u / upd_threads_per_cell(count); }
constexpr uint32_t kMRayEmpty = 0xFFFFFFFFu;  // (= kRayEmpty, fdm_raycast.hpp)
constexpr int kLayTab = 64;           // layer pointers an update block keeps in LDS for its all-layer wipes (MUpdLds::lay)
template <bool COL, bool RAY>
struct MUpdLds {
  MEvent ev[kEvCap];
  union {
    MObs ob[kEvCap];
    // the cell masks on their way from the cell's threads to everyone who numbers or applies its events, [group][cell of
    // the block] (tpc x cpb = 256 either way): the four scan bits of a group, in place.  Read between the barrier behind
    // round trip 1 and the first barrier of the round loop, which is where ob's first writer waits
    struct { uint32_t tpart[256], rpart[RAY ? 256 : 1]; } mk;
  };
  uint32_t rgb[COL ? kEvCap : 1];
  uint32_t rcnt[RAY ? kMaxBatch * kUpdCells : 1], rmin[RAY ? kMaxBatch * kUpdCells : 1];  // [scan][cell of the block]
  unsigned s_t[4];
  // all_layers[0 .. kLayTab), copied by wavefront 1 during round trip 1: the owners' wipe of vacated cells reads its
  // pointers here and not from global memory behind the walk.  (Not with RAY: those blocks' LDS is their occupancy.)
  float* lay[RAY ? 1 : kLayTab];
};
template <bool COL, bool RAY>
constexpr unsigned kMLdsBytes = sizeof(MUpdLds<COL, RAY>) > sizeof(MBinLds) ? sizeof(MUpdLds<COL, RAY>) : sizeof(MBinLds);

// ---------------------------------------------------------------------------------------------
// crop half: SCOUT blocks of the NEXT batch's scans — does scan k hold a point that survives the crops (then it moves a
// LOCAL map, fastdem.cpp:138-145)?  kMScout blocks per scan walk it with a grid stride, kMBlock points per block and
// step, and leave at the first step in which any thread of the block sees a survivor: for a real scan that is the
// first step, only a scan without survivors (a covered sensor) is read to its end.  (Round 3 ran the crops over EVERY
// point of the next batch here — as many blocks again as the bin half, a third of the launch's blocks and of its input
// traffic, for sixteen bits: configs[2] 10.5 us per scan, VERDICT r03 #6.)
constexpr unsigned kMScout = 4u;
__device__ __forceinline__ void mcrop_body(const MCrop& Cn, const MCommon& K, const unsigned k, const unsigned sb) {
  unsigned n = Cn.s[k].n;
  const float* px_ = Cn.s[k].px;
  const float* py_ = Cn.s[k].py;
  const float* pz_ = Cn.s[k].pz;
  FDM_SGPR_NOW4(n, px_, py_, pz_);  // the scan's record: one batch, one wait (the crops' limits join it)
  const MView V = mview(K, nullptr, nullptr);
  const float* __restrict__ const px = px_;
  const float* __restrict__ const py = py_;
  const float* __restrict__ const pz = pz_;
#pragma unroll 1
  for (unsigned i0 = sb * kMBlock; i0 < n; i0 += kMScout * kMBlock) {  // (block-uniform)
    bool pass = false;
#pragma unroll
    for (int h = 0; h < kMPts; ++h) {
      const unsigned i = i0 + unsigned(h) * 256u + threadIdx.x;
      if (i < n) {
        float x = px[i], y = py[i], z = pz[i], w;
        pass = mcrops(V, x, y, z, w) || pass;
      }
    }
    if (__syncthreads_or(pass ? 1 : 0)) {
      if (threadIdx.x == 0) atomicOr(&Cn.ms->flags[0], 1u << k);  // (<= kMScout per scan)
      return;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The chain of LOCAL-mode moves of a batch, walked ONCE and one launch ahead.  Scan k is binned against the geometry
// after the moves of scans 0 .. k - 1, and every bin block used to walk that chain itself behind its point loads — up to
// fifteen dependent moves (~0.3 us each on a full chip: every second pose of a robot advancing half a cell per scan sits
// on a rounding tie and takes the reference's subtract + divide), 4.5 us for the blocks of a batch's sixteenth scan, which
// is what ended the launch.  One extra block of the scout rows (the WALKER) walks the NEXT batch's chain while this
// launch runs — geometry before / after every scan's move into MState::PE / PC — assuming every scan of it passes the
// crops (the scouts' answer is not complete before the launch ends; a scan with no surviving point is a covered sensor).
// A bin block whose scan's predecessors did pass takes PE[k] / PC[k] (two loads that leave with its point loads); if
// one did not, it walks as before.  Measured (16 scans per launch): configs[2] (P2, colour; 87 us launches) 5.40 -> 4.79 us
// per scan; configs[1] (Kalman; 16 us launches) unchanged on streamed inputs and SLOWER on cache-resident ones (1.02 ->
// 1.30 us per scan): that launch is bound by its memory-side atomics, the chains staggered the sixteen rows of bin blocks
// by 0.3 us each and left the update half the first microseconds — all rows at once make the update half the last to
// finish (phase stamps: 13.6 -> 17.1 us; measured again with the compact winner slots of mbin_body's merge: rocprof
// 15.6 -> 17.6 us per launch, profiles/r07).  Taking the walker's chain only in the rows of the longest chains keeps the
// stagger of the early rows and takes the tail off the late ones: scans >= 12 of a 16-scan Kalman batch
// (MCommon::walk_from, kKalmanWalkFrom; profiles/r07: 24.2 -> 25.2 G pts/s against 10, 13 or 14 within 0.4 %).  That
// stagger was worth something only while a record cost four memory-side requests: since the flush sends a record's aux
// words as one (profiles/r19/flush: 123 K -> 71 K atomic requests per launch) every row takes the walker's chain —
// kKalmanWalkFrom 0: 31.5 -> 34.8 G pts/s against 12, 33.8 with 8.  So by
// default the walker serves every scan with the quantile estimator and with Kalman without the ray stage, none
// with Kalman and raycasting (option "batch_walk": -1 automatic, 0 off, 1 on for every scan).  The walk itself is the reference's sequence, scan by scan: geometry before scan
// k + 1 = scan k's candidate if scan k moved the map, else unchanged — the same numbers the per-block walk produces
// (it defers the index wrap of short moves, which yields the candidate's wrapped index).
//
// Geometry before the first scan of a batch, from the state of the batch before it (complete) or the geometry ring.
// (prev is always readable — MBin::prev — so both sources are loaded together and the choice is a select)
__device__ __forceinline__ DevGeom mbatch_start(const MState* __restrict__ prev, unsigned prev_count, bool has_prev,
                                                unsigned scan_no0, const MCommon& K, const DevState* __restrict__ st) {
  const unsigned pk = (prev_count - 1u) & unsigned(kMaxBatch - 1);  // (1 .. kMaxBatch: the mask only keeps a stray count inside the arrays)
  const DevGeom ring = st->geom[scan_no0 & 3u];
  DevGeom g = prev->E[pk];
  const DevCand c = prev->C[pk];
  const unsigned f = prev->flags[0];
  if (K.do_move && (!K.gate_on_filter || ((f >> pk) & 1u) != 0u)) { g.px = c.px; g.py = c.py; g.sr = c.sr; g.sc = c.sc; }
  return has_prev ? g : ring;
}
// The arithmetic of a chain of moves, shared by the walker (mwalk_batch) and the bin blocks' own walk (mbin_body): both
// must produce the reference's numbers, so there is one copy.  move() snaps the position to the grid p0 + integer * res, so
// in exact arithmetic the TOTAL shift after scan j's move is round((pose_j - p0) / res) whatever happened before it: lane j
// of a wavefront rounds its scan's pose ONCE against the chain's start (mchain_nearest), with move_candidate_fast's own
// margins (1e-4 cell off a rounding tie; the accumulated position differs from p0 + V res by ~1e-10 cell at most), and the
// walk takes scan j's shift as that total minus the cells shifted so far.  A pose within the margin of a tie (a robot
// advancing half a cell per scan) takes the reference's subtract + divide against the position accumulated so far, at its
// place in the walk (mchain_shift).
//
// lane j's double, in every lane
__device__ __forceinline__ double lane_f64(double v, unsigned j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), int(j));
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), int(j));
  return __hiloint2double(hi, lo);
}
// t = a rounded half away from zero; is it the reference's shift for certain?  (a = (pose - p0) / res, estimated)
__device__ __forceinline__ bool mchain_nearest(double a, double p0, int& t) {
  t = 0;
  if (!(fabs(p0) < 1.0e7)) return false;
  if (fabs(a) <= 1e-4) return true;
  const double ue = a + 0.5 * (a > 0 ? 1 : -1);
  t = static_cast<int>(ue);
  const double f = fabs(ue - double(t));
  return f > 1e-4 && f < 1.0 - 1e-4 && fabs(ue) < 1.0e6;
}
// scan j's move along one axis against the position walked so far: p, v cells from the chain's start.  Lane j holds
// scan j's pose and its rounding t; bit j of `sure`: that rounding is off every tie
__device__ __forceinline__ int mchain_shift(unsigned sure, int t, double pose, unsigned j, double p, int v, const GeomConst& G) {
  if ((sure >> j) & 1u) return __builtin_amdgcn_readlane(t, int(j)) - v;
  // GridMap::move's own arithmetic (the quotient correctly rounded: div_by_res)
  const double q = div_by_res(lane_f64(pose, j) - p, G.res, G.inv_res);
  return static_cast<int>(q + 0.5 * (q > 0 ? 1 : -1));
}
// One batch's chain from `g` on (every lane of one wavefront, uniformly; lane j holds scan j's pose): E / C of every scan
// into `out` (nullable), the last scan's returned.
__device__ __forceinline__ void mwalk_batch(DevGeom g, const unsigned count, const double* __restrict__ rx,
                                            const double* __restrict__ ry, const unsigned passmask, const MCommon& K,
                                            const GeomConst& G, MState* __restrict__ out, DevGeom& e_last, DevCand& c_last) {
  const unsigned lane = threadIdx.x & 63u;
  double pose_x = 0.0, pose_y = 0.0;
  if (lane < count) { pose_x = rx[lane]; pose_y = ry[lane]; }
  int tx = 0, ty = 0;
  const bool sx = mchain_nearest((pose_x - g.px) * G.inv_res, g.px, tx), sy = mchain_nearest((pose_y - g.py) * G.inv_res, g.py, ty);
  const unsigned sure_x = K.dbg == 3 ? 0u : uni(unsigned(__ballot(sx))), sure_y = K.dbg == 3 ? 0u : uni(unsigned(__ballot(sy)));
  int vx = 0, vy = 0;
  DevCand c;
  c.px = g.px; c.py = g.py; c.sr = g.sr; c.sc = g.sc; c.shr = 0; c.shc = 0;
#pragma unroll 1
  for (unsigned k = 0; k < count; ++k) {
    const int dx = mchain_shift(sure_x, tx, pose_x, k, g.px, vx, G);
    const int dy = mchain_shift(sure_y, ty, pose_y, k, g.py, vy, G);
    c.sr = g.sr - dx; c.sc = g.sc - dy;
    wrap_index(c.sr, G.rows);
    wrap_index(c.sc, G.cols);
    c.px = g.px + double(dx) * G.res;
    c.py = g.py + double(dy) * G.res;
    c.shr = -dx; c.shc = -dy;
    if (out && lane == 0u) { out->PE[k] = g; out->PC[k] = c; }
    e_last = g;
    if ((passmask >> k) & 1u) {  // GridMap::move: the map is where the candidate says
      g.px = c.px; g.py = c.py; g.sr = c.sr; g.sc = c.sc;
      vx += dx; vy += dy;
    }
  }
  c_last = c;
}
// The walker block (first wavefront): chain of the scouted batch Cn into Cn.ms->PE / PC.
__device__ __forceinline__ void mwalk_body(const MBin& B, const MCrop& Cn, const MCommon& K, const GeomConst& G,
                                           const DevState* __restrict__ st, const unsigned b_count, const unsigned c_count) {
  if (threadIdx.x >= 64u || !K.do_move || !K.walk || K.dbg == 2) return;
  const unsigned lane = threadIdx.x & 63u;
  DevGeom g;
  if (b_count) {  // behind the batch this launch bins: its own chain as pre-walked if its scouts agreed, else walked here
    const unsigned act = K.gate_on_filter ? uni(B.ms->flags[0]) : 0xFFFFFFFFu, pre = uni(B.ms->flags[1]);
    const bool pre_valid = uni(B.ms->flags[2]) != 0u;
    const unsigned last = b_count - 1u;
    DevGeom e_l;
    DevCand c_l;
    if (pre_valid && ((pre ^ act) & lowbits(last)) == 0u) {
      e_l = B.ms->PE[last];
      c_l = B.ms->PC[last];
    } else {
      mwalk_batch(mbatch_start(B.prev, B.prev_count, B.has_prev != 0u, B.scan_no0, K, st), b_count, B.robot_x, B.robot_y, act,
                  K, G, nullptr, e_l, c_l);
    }
    g = e_l;
    if ((act >> last) & 1u) { g.px = c_l.px; g.py = c_l.py; g.sr = c_l.sr; g.sc = c_l.sc; }
  } else {
    g = mbatch_start(Cn.prev, Cn.prev_count, Cn.has_prev != 0u, Cn.scan_no0, K, st);
  }
  DevGeom e_l;
  DevCand c_l;
  mwalk_batch(g, c_count, Cn.robot_x, Cn.robot_y, 0xFFFFFFFFu, K, G, Cn.ms, e_l, c_l);
  if (lane == 0u) { Cn.ms->flags[1] = lowbits(c_count); Cn.ms->flags[2] = 1u; }
}

// ---------------------------------------------------------------------------------------------
// bin half: block `bid` of the batch's bin grid.  CH: bit 0 intensity, bit 1 colour (compile-time, as k_bin's).
template <int CH, bool RAY>
__device__ __forceinline__ void mbin_body(const MBin& B_, const MCommon& K_, const GeomConst& G_,
                                          DevState* __restrict__ st, const unsigned ncell, const unsigned k,
                                          const unsigned lb, MBinLds& S) {
  // (scan k of the batch and the block's number inside the scan come straight from the grid: nothing to look up
  // before the point loads can leave)
  constexpr bool has_int = (CH & 1) != 0, has_col = (CH & 2) != 0;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // The block's ONE batch of scalar loads behind the head: scan k's record (MBinScan: one line) and what the first
  // wavefront's geometry loads go through.  All of it is independent of everything but k, so it leaves together and the
  // wavefront waits once; the surplus blocks of a short row leave behind that wait, not in front of the pointer loads.
  // (prgb, pvar, first_block and the transforms are not needed before the point loads: they stay where they are used.)
  const MBinScan& R = B_.s[k];
  unsigned n_ = R.n;
  const float* px_ = R.px;
  const float* py_ = R.py;
  const float* pz_ = R.pz;
  const float* pint_ = has_int ? R.pint : nullptr;
  MState* ms_ = B_.ms;
  const MState* prev_ = B_.prev;
  unsigned prev_count_ = B_.prev_count, has_prev_ = B_.has_prev, scan_no0_ = B_.scan_no0;
  FDM_SGPR_NOW10(n_, px_, py_, pz_, pint_, ms_, prev_, prev_count_, has_prev_, scan_no0_);
  const unsigned n = n_;
  if (lb >= (n + kMBlock - 1u) / kMBlock) return;  // (block-uniform)
  const MBin& B = kernarg_from_here(B_);  // (everything else of the arguments is read behind the point loads' issue)
  const MCommon& K = kernarg_from_here(K_);
  const GeomConst& G = kernarg_from_here(G_);
  MState* const ms = ms_;
  const MState* const prev = prev_;
  const bool has_prev = has_prev_ != 0u;
  const MView V = mview(K, R.t.Twb, R.t.R);
  const float* __restrict__ const px = px_;
  const float* __restrict__ const py = py_;
  const float* __restrict__ const pz = pz_;
  const float* __restrict__ const pint = pint_;

  // (the poses and the geometry the chain starts from leave before the point loads: loads return in order, and the
  // walk below waits for these; the previous batch's candidate is fetched whether or not it will apply — one round
  // trip instead of flag -> candidate)
  double pose_x = 0.0, pose_y = 0.0;
  DevGeom g_start, g_pre;
  DevCand c_prev, c_pre;
  unsigned f_prev = 0u, w_pre = 0u, w_valid = 0u;
  g_start.px = g_start.py = 0.0; g_start.sr = g_start.sc = 0; g_start.pad0 = g_start.pad1 = 0;
  c_prev.px = c_prev.py = 0.0; c_prev.sr = c_prev.sc = c_prev.shr = c_prev.shc = 0;
  g_pre = g_start;
  c_pre = c_prev;
  if (threadIdx.x < 64u) {
    // (the chain as the walker block of the previous launch left it: used if the scouts confirmed what it assumed)
    w_pre = ms->flags[1];
    w_valid = ms->flags[2];
    g_pre = ms->PE[k];
    c_pre = ms->PC[k];
    if (lane <= k) { pose_x = B.robot_x[lane]; pose_y = B.robot_y[lane]; }
    // (the chain's start: every address is known from the block's one batch of arguments — prev is always readable —
    // so the loads leave unconditionally and together; which geometry applies is a select on two addresses, both
    // valid, and costs no register and no wait in front of the point loads)
    const unsigned pk = (prev_count_ - 1u) & unsigned(kMaxBatch - 1);
    const DevGeom* const g_from = has_prev ? &prev->E[pk] : &st->geom[scan_no0_ & 3u];
    g_start = *g_from;
    c_prev = prev->C[pk];
    f_prev = prev->flags[0];
  }
  const unsigned i0 = lb * kMBlock + threadIdx.x;  // the thread's points: i0, i0 + 256 (two coalesced sweeps)
  float xs[kMPts], ys[kMPts], zs[kMPts], vs[kMPts];
#pragma unroll
  for (int h = 0; h < kMPts; ++h) {  // the loads go out first
    const unsigned i = i0 + unsigned(h) * 256u;
    xs[h] = ys[h] = zs[h] = vs[h] = 0.f;
    if (i < n) {
      xs[h] = px[i];
      ys[h] = py[i];
      zs[h] = pz[i];
      if (has_int) vs[h] = pint[i];
    }
  }
#if FDM_MB_PHASES == 2  // (variant: kernel arguments read + loads issued | loads back | chain walked)
  FDM_PHASE(0);
#endif
#pragma unroll
  for (int h = 0; h < kMPts; ++h) {
    const unsigned t = threadIdx.x + unsigned(h) * 256u;
    S.t_key[t] = kEmptyKey;
    S.t_cell[t] = kEmptyCell;
    S.t_zmx[t] = 0u; S.t_imx[t] = 0u; S.t_fst[t] = kNoIdx; S.t_lst[t] = 0u;
  }
  if (threadIdx.x == 0) S.s_nrec = 0u;
#if FDM_MB_PHASES == 2
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  FDM_PHASE(1);
#endif
  // The chain of moves up to this scan, given which of the earlier scans moved the map — walked by the whole first
  // wavefront (lane j holds scan j's pose: mchain_nearest, mchain_shift), because a serial instruction costs ~10 ns on a
  // full chip and a block of the batch's last scan used to spend 6.6 us here.
  auto chain = [&](unsigned passmask) {  // (every lane of the first wavefront, uniformly)
    if (K.do_move && K.walk && K.dbg != 2 && K.dbg != 3 && k >= unsigned(K.walk_from) && uni(w_valid) != 0u &&
        ((uni(w_pre) ^ passmask) & lowbits(k)) == 0u) {  // pre-walked (mwalk_body): nothing to walk
      if (threadIdx.x == 0) {
        S.s_cand = c_pre;
        if (lb == 0u) { ms->E[k] = g_pre; ms->C[k] = c_pre; }
      }
      return;
    }
    DevGeom g = g_start;
    if (has_prev) {  // what the update of the previous batch (the other half of this launch) is about to commit
      const unsigned pk = (prev_count_ - 1u) & unsigned(kMaxBatch - 1);
      if (K.do_move && (!K.gate_on_filter || ((f_prev >> pk) & 1u) != 0u)) {
        g.px = c_prev.px; g.py = c_prev.py; g.sr = c_prev.sr; g.sc = c_prev.sc;
      }
    }
    DevCand c;
    c.px = g.px; c.py = g.py; c.sr = g.sr; c.sc = g.sc; c.shr = 0; c.shc = 0;
    if (K.do_move) {
      int tx = 0, ty = 0;
  const bool sx = mchain_nearest((pose_x - g.px) * G.inv_res, g.px, tx), sy = mchain_nearest((pose_y - g.py) * G.inv_res, g.py, ty);
  const unsigned sure_x = K.dbg == 3 ? 0u : uni(unsigned(__ballot(sx))), sure_y = K.dbg == 3 ? 0u : uni(unsigned(__ballot(sy)));
      int vx = 0, vy = 0;  // total shift so far, in cells
      auto shift_of = [&](unsigned j, int& dx, int& dy) {  // scan j's move against the geometry walked so far
        dx = mchain_shift(sure_x, tx, pose_x, j, g.px, vx, G);
        dy = mchain_shift(sure_y, ty, pose_y, j, g.py, vy, G);
      };
      unsigned m = K.dbg == 2 ? 0u : ((K.gate_on_filter ? passmask : 0xFFFFFFFFu) & lowbits(k));  // the moves ahead of scan k
      bool unwrapped = false;
      while (m) {  // (a scan that returned before its move is not in the mask)
        const unsigned j = unsigned(__ffs(int(m))) - 1u;
        m &= m - 1u;
        int dx, dy;
        shift_of(j, dx, dy);
        // The start index is wrapped ONCE behind the walk.  For a shift of fewer cells than the map has,
        // wrapIndexToRange returns the representative in [0, size) of its argument modulo size — wrapping after every
        // move and reducing the sum are then the same number, and the per-move wrap was a third of the walk's serial
        // instructions (0.35 us per move on a full chip: 5 us for the blocks of a batch's sixteenth scan, which is what
        // ended the launch).  A shift of >= size cells (a jump beyond the map) takes the reference's own function at its
        // place in the walk, quirks included (it returns `size` for an argument of -2 size).
        const bool small = unsigned(dx + G.rows - 1) < unsigned(2 * G.rows - 1) && unsigned(dy + G.cols - 1) < unsigned(2 * G.cols - 1);
        if (!small) {
          if (unwrapped) {
            g.sr %= G.rows; if (g.sr < 0) g.sr += G.rows;
            g.sc %= G.cols; if (g.sc < 0) g.sc += G.cols;
            unwrapped = false;
          }
          g.sr -= dx; g.sc -= dy;
          wrap_index(g.sr, G.rows);
          wrap_index(g.sc, G.cols);
        } else {
          g.sr -= dx; g.sc -= dy;
          unwrapped = true;
        }
        g.px = g.px + double(dx) * G.res;
        g.py = g.py + double(dy) * G.res;
        vx += dx; vy += dy;
      }
      if (unwrapped) {  // (the small shifts accumulated since the last wrap)
        g.sr %= G.rows; if (g.sr < 0) g.sr += G.rows;
        g.sc %= G.cols; if (g.sc < 0) g.sc += G.cols;
      }
      int dx, dy;
      shift_of(k, dx, dy);
      c.sr = g.sr - dx; c.sc = g.sc - dy;
      wrap_index(c.sr, G.rows);
      wrap_index(c.sc, G.cols);
      c.px = g.px + double(dx) * G.res;
      c.py = g.py + double(dy) * G.res;
      c.shr = -dx; c.shc = -dy;
    }
    if (threadIdx.x == 0) {
      S.s_cand = c;
      if (lb == 0u) { ms->E[k] = g; ms->C[k] = c; }
    }
  };
  // (which of the scans ahead moved the map is known before the launch starts: the scout blocks of the previous launch —
  // or a small launch of their own ahead of a call's first batch — left it in the state word.  The walk runs in the
  // shadow of the point loads; nothing is published, nothing is polled)
  const bool gated = K.do_move && K.gate_on_filter;
  if (threadIdx.x < 64u) chain((gated && k > 0u) ? uni(ms->flags[0]) : 0xFFFFFFFFu);

#if FDM_MB_PHASES == 2
  FDM_PHASE(2);
#else
  FDM_PHASE(0);  // table initialised, chain walked (the point loads are still in flight; vmcnt returns in order)
#endif
  bool pass[kMPts];
  unsigned npw = 0u;
#pragma unroll
  for (int h = 0; h < kMPts; ++h) {
    const unsigned i = i0 + unsigned(h) * 256u;
    const float sx = xs[h], sy = ys[h], sz = zs[h];
    float w = 1.0f;
    pass[h] = false;
    if (i < n) pass[h] = mcrops(V, xs[h], ys[h], zs[h], w);
    transform4_affine(V.Twb12, xs[h], ys[h], zs[h], w);
    if (RAY && B.cap && i < n) {  // the raycasting stage's input: the preprocessed cloud by point index (as k_bin's capture)
      const size_t at = size_t(k) * B.obs_stride + i, plane = size_t(kMaxBatch) * B.obs_stride;
      B.cap[at] = pass[h] ? xs[h] : __uint_as_float(0x7FC00000u);
      B.cap[plane + at] = ys[h];
      B.cap[2u * plane + at] = zs[h];
    }
    S.s_pt[threadIdx.x + unsigned(h) * 256u] = make_float4(sx, sy, sz, zs[h]);
    npw += unsigned(__popcll(__ballot(pass[h])));
  }
  if (lane == 0u) S.s_pass[wave] = npw;
#if FDM_MB_PHASES != 2
  FDM_PHASE(1);  // points arrived, crops + both transforms done
#endif
  __syncthreads();  // table, s_pt, s_pass, s_cand
  const unsigned np = S.s_pass[0] + S.s_pass[1] + S.s_pass[2] + S.s_pass[3];
  const DevCand cand = S.s_cand;

  unsigned long long* const S_key = B.key + size_t(k) * ncell;
  uint32_t* const S_aux = reinterpret_cast<uint32_t*>(B.aux + size_t(k) * ncell);
  uint32_t* const S_zs = reinterpret_cast<uint32_t*>(B.zs + size_t(k) * ncell);
  float2* const S_obs = B.obs + size_t(k) * B.obs_stride;
  uint32_t* const S_cobs = B.cobs + size_t(k) * B.obs_stride;
  // (the rest of the scan's record, read once here and not per record of the flush)
  const uint32_t* __restrict__ const prgb = has_col ? R.prgb : nullptr;
  const float* __restrict__ const pvar = R.pvar;

  // one cell's reduction goes to the scan's scratch; the merging thread also leaves what the update needs of the
  // block-local winner / last point in the block's SLOT for the cell: slot = lb * kMBlock + j, j = the number the
  // cell's record got when its table slot was claimed (the fold below).  The slot replaces the point index in the low
  // word of the key and in aux.w, so that a block's observations form one contiguous run (a few lines) instead of one
  // isolated store per cell, and the update's gather of neighbouring cells shares lines.  Order is kept where it
  // matters: block lb owns points [lb kMBlock, lb kMBlock + kMBlock) and holds ONE entry per cell, so between two
  // blocks a lower slot on equal ord(z) is still the earlier point (strict "<", elevation_mapping.cpp:41-92), and a
  // higher slot is still the later last point.  The order of the records INSIDE a block is the order in which its
  // wavefronts reached the counter — it depends on timing, and no output may depend on it: a cell never compares two
  // slots of one block.  j < the block's claims <= its inside points, so slot < n: inside the scan's slot of obs / cobs
  // and never kNoIdx.  fst and zs stay point indices (never gathered).
  // The key half of a record (one lane per record): the key's atomic, the colour and the observation of the slot.
  auto merge_key = [&](uint32_t c, unsigned long long key, uint32_t lst, uint32_t slot) {
    const uint32_t idx = uint32_t(key);  // the block-local winner's point index (kNoIdx: no finite z below FLT_MAX)
    if (idx != kNoIdx) key = (key & 0xFFFFFFFF00000000ull) | slot;
    atomicMin(&S_key[c], key);
    if (has_col) S_cobs[slot] = prgb[lst];
    if (idx != kNoIdx) {
      const float4 p = S.s_pt[idx - lb * kMBlock];
      float var = 0.0f;  // CellObservation default (elevation_mapping.hpp:26-34)
      if (K.has_var) var = pvar[idx];
      else if (K.integrate_mode) var = sigma_z2(V, p.x, p.y, p.z);
      S_obs[slot] = make_float2(p.w, var);
    }
  };

  // getIndex on a fixed-point estimate, the reference's fp64 arithmetic only for the lanes within 2^-shift cell of
  // a cell edge (axis_fast / axis_exact, as k_tbin); every point then folds straight into the block's LDS cell
  // table — LDS atomics are cheap, the cross-lane run merge of k_bin costs more instructions than it saves here
  unsigned niw = 0u;
  bool any_glob = false;
  const bool any_start = cand.sr != 0 || cand.sc != 0;
  const double off_r = (G.half_x + cand.px) * G.inv_res_k, off_c = (G.half_y + cand.py) * G.inv_res_k;
  // what each of the thread's points contributes to its cell, and whether the point goes to the table itself
  int cells[kMPts];
  bool commit[kMPts];
  unsigned long long keys[kMPts];
  uint32_t zmxs[kMPts], imxs[kMPts], fsts[kMPts], lsts[kMPts];
#pragma unroll
  for (int h = 0; h < kMPts; ++h) {
    const unsigned i = i0 + unsigned(h) * 256u;
    const float x = xs[h], y = ys[h], z = zs[h], vint = vs[h];
    bool sure_r, sure_c;
    int kr = axis_fast(double(x), off_r, G.inv_res_k, G.idx_shift, G.rows, sure_r);
    int kc = axis_fast(double(y), off_c, G.inv_res_k, G.idx_shift, G.cols, sure_c);
    bool in = pass[h];
    if (__ballot(pass[h] && !(sure_r && sure_c))) {  // wave-uniform; well under a percent of the wavefronts
      if (pass[h] && !sure_r) in = axis_exact(double(x), cand.px, G.half_x, G.len_x, G.res, kr);
      if (in && !sure_c) in = axis_exact(double(y), cand.py, G.half_y, G.len_y, G.res, kc);
    }
    const bool okr = axis_wrap(kr, cand.sr, any_start, G.rows);  // (both axes are evaluated, as getIndex does)
    const bool okc = axis_wrap(kc, cand.sc, any_start, G.cols);
    const bool in_map = in && okr && okc;
    const int lr = kr - G.o_r0, lc = kc - G.o_c0;
    const bool inside = in_map && unsigned(lr) < unsigned(G.o_rows) && unsigned(lc) < unsigned(G.o_cols);
    const int cell = (kc - G.s_c0) * G.s_rows + (kr - G.s_r0);
    any_glob = any_glob || in_map;
    if (inside) {
      if (z == 0.0f) atomicMin(S_zs + size_t(cell) * 2, (i << 1) | (__float_as_uint(z) >> 31));
      if (has_int && vint == 0.0f) atomicMin(S_zs + size_t(cell) * 2 + 1, (i << 1) | (__float_as_uint(vint) >> 31));
    }
    unsigned long long key = kEmptyKey;
    uint32_t zmx = 0u, imx = 0u, fst = kNoIdx, lst = 0u;
    if (inside) {
      key = make_key(z, i);
      zmx = make_zmax(z);
      if (has_int) {
        const bool vnan = isnan(vint);
        imx = vnan ? 0u : ord(vint);
        fst = (i << 1) | (vnan ? 1u : 0u);
      }
      lst = i;
    }
    // Neighbouring lanes are neighbouring points: on an image-ordered cloud (RGB-D rows) they fall into the same cell
    // in runs of ten or twenty, and every LDS atomic of such a wavefront serialises on a handful of table slots
    // (SQ_LDS_ADDR_CONFLICT, profiles/r04/pmc_lds_mbatch_halves.txt).  A wavefront whose runs are long merges them in
    // registers first (segmented scan over runs of equal cell, as k_bin does) and only the run TAILS touch the table;
    // a firing-order LiDAR scan (neighbouring lanes = different beams: every lane its own run) skips the merge —
    // decided per wavefront from two ballots.  min / max are idempotent: either way the table ends up the same.
    commit[h] = inside;
    {
      const int prev_cell = __shfl_up(inside ? cell : -1, 1);
      const bool head = inside && (lane == 0u || prev_cell != cell);
      const unsigned n_in = unsigned(__popcll(__ballot(inside))), n_runs = unsigned(__popcll(__ballot(head)));
      if (n_runs * 4u <= n_in) {  // (wave-uniform) average run >= 4 points
        const int mcell = inside ? cell : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int ocell = __shfl_up(mcell, d);
          const unsigned long long okey = __shfl_up(key, d);
          const uint32_t ozmx = __shfl_up(zmx, d);
          const uint32_t oimx = has_int ? __shfl_up(imx, d) : 0u;
          const uint32_t ofst = has_int ? __shfl_up(fst, d) : kNoIdx;
          if (int(lane) >= d && ocell == mcell && inside) {
            key = okey < key ? okey : key;
            zmx = ozmx > zmx ? ozmx : zmx;
            imx = oimx > imx ? oimx : imx;
            fst = ofst < fst ? ofst : fst;
          }
        }
        // (lst: the tail of a run is its highest point index already)
        const int next_cell = __shfl_down(mcell, 1);
        commit[h] = inside && (lane == 63u || next_cell != cell);
      }
    }
    cells[h] = cell; keys[h] = key; zmxs[h] = zmx; imxs[h] = imx; fsts[h] = fst; lsts[h] = lst;
    niw += unsigned(__popcll(__ballot(inside)));
  }
  // ---- fold: the thread's points probe the table in ONE batch (the probes' LDS round trips overlap; a second look
  // only on a real collision), then the atomics.  The lane whose probe found the slot EMPTY has claimed it — exactly
  // one lane per cell of the block — and numbers the cell's record there: a ballot of the claims and one LDS add per
  // wavefront for all its points together (as fdm_tbin2.hpp).  No compaction pass over the table behind the fold.
  uint32_t hs[kMPts], seen[kMPts];
#pragma unroll
  for (int h = 0; h < kMPts; ++h) {
#ifdef FDM_X_MHASH  // (measurement build, profiles/r06/batch_max.txt: a multiplicative hash instead of cell mod 512)
    hs[h] = (uint32_t(cells[h]) * 2654435761u) >> 23;
#else
    hs[h] = uint32_t(cells[h]) & (kMBlock - 1u);
#endif
    seen[h] = uint32_t(cells[h]);
    if (commit[h]) seen[h] = atomicCAS(&S.t_cell[hs[h]], kEmptyCell, uint32_t(cells[h]));
  }
  unsigned long long claims[kMPts];
  unsigned n_claims = 0u;
#pragma unroll
  for (int h = 0; h < kMPts; ++h) {
    bool claimed = commit[h] && seen[h] == kEmptyCell;
    if (commit[h] && !claimed && seen[h] != uint32_t(cells[h])) {  // a real collision: linear probing
      uint32_t hh = hs[h];
      while (true) {
        hh = (hh + 1) & (kMBlock - 1u);
        const uint32_t prev = atomicCAS(&S.t_cell[hh], kEmptyCell, uint32_t(cells[h]));
        claimed = prev == kEmptyCell;
        if (claimed || prev == uint32_t(cells[h])) break;
      }
      hs[h] = hh;
    }
    claims[h] = __ballot(claimed);
    n_claims += unsigned(__popcll(claims[h]));
    if (commit[h]) {
      atomicMin(&S.t_key[hs[h]], keys[h]);
      atomicMax(&S.t_zmx[hs[h]], zmxs[h]);  // (max with 0: no-op)
      if (has_int) {
        atomicMax(&S.t_imx[hs[h]], imxs[h]);
        atomicMin(&S.t_fst[hs[h]], fsts[h]);
      }
      if (has_col) atomicMax(&S.t_lst[hs[h]], lsts[h]);
    }
  }
  if (n_claims) {  // (wave-uniform) claims <= the block's inside points <= kMBlock: the list cannot overflow
    unsigned base = 0u;
    if (lane == 0u) base = atomicAdd(&S.s_nrec, n_claims);
    base = uni(base);
#pragma unroll
    for (int h = 0; h < kMPts; ++h) {
      if ((claims[h] >> lane) & 1ull) S.s_list[base + lane_rank(claims[h])] = uint16_t(hs[h]);
      base += unsigned(__popcll(claims[h]));
    }
  }
  // (the ballot BEFORE the lane test: inside `if (lane == 0)` it would see lane 0 alone — a small scan whose first
  // point lies outside the map then never reported "observed", and the obstacle layer kept the previous scan's values)
  const bool wave_glob = __ballot(any_glob) != 0ull;
  if (lane == 0u) {
    S.s_in[wave] = niw;
    if (wave_glob) ms->inside[k] = 1u;
  }
  // ---- flush: the block's records in claim order, so that the sigma_z^2 evaluation and the memory-side atomics of a
  // block's ~100 cells keep two wavefronts busy instead of four, twice ----
#if FDM_MB_PHASES != 2
  FDM_PHASE(2);  // index + LDS fold done
#endif
  __syncthreads();  // the table, the record list and its count are complete
  // A pass takes 64 records.  Their aux words leave in ONE atomic instruction, four adjacent lanes per record (lane
  // 4 r + w: word w of record r, 16 contiguous bytes — the memory side takes a record as one request where three
  // instructions were three, scripts/ubench/atomic_rec.hip).  Every word of the scratch is a maximum and its clean value
  // is 0: fst travels inverted (max of ~fst = ~ min of fst; kNoIdx -> 0), and a lane whose word is 0 has nothing to
  // send — a channel the instantiation lacks, no finite intensity, make_zmax's 0.  The key halves of the pass go
  // through ONE wavefront, another one in every pass and the last in the first (the records of a typical block fill
  // the lower wavefronts with aux words): neither part waits for the other.
  const unsigned n_occ = K.dbg == 1 ? 0u : uni(S.s_nrec);  // (dbg_batch 1: no merge at all)
  for (unsigned j0 = 0u, p = 0u; j0 < n_occ; j0 += 64u, ++p) {
    const unsigned r = j0 + (threadIdx.x >> 2), w = threadIdx.x & 3u;
    if (r < n_occ) {
      const unsigned t = S.s_list[r];
      const uint32_t* const src = w == 0u ? S.t_zmx : w == 1u ? S.t_imx : S.t_fst;
      uint32_t v = src[t];
      if (w == 2u) v = ~v;
      if (w == 3u) v = has_col ? lb * kMBlock + r : 0u;  // (the slot: a later block's is higher)
      if (v) atomicMax(S_aux + size_t(S.t_cell[t]) * 4 + w, v);
    }
    if (wave == ((3u - p) & 3u)) {  // (wave-uniform)
      const unsigned j = j0 + lane;
      if (j < n_occ) {
        const unsigned t = S.s_list[j];
        merge_key(S.t_cell[t], S.t_key[t], S.t_lst[t], lb * kMBlock + j);
      }
    }
  }
  if (threadIdx.x == 0) {
    const unsigned ni = S.s_in[0] + S.s_in[1] + S.s_in[2] + S.s_in[3];
    B.bin_part[R.first_block + lb] =(unsigned long long)np | ((unsigned long long)ni << 32);
  }
}

// ---------------------------------------------------------------------------------------------
// update half: kUpdCells cells of the map (memory order), every scan of the batch.  Four threads per cell — thread
// q * cpb + c looks after cell c in scans 4 q .. 4 q + 3 — so that a block holds at most 1024 events (two rounds of
// the exchange) and the densest corner of the map (every cell touched by every scan) is a chain as short as any
// other; the cell's own thread (q == 0) applies the events.  Group-major, so the owners are dense: with 64 cells per
// block wavefront q IS group q and wavefront 0 applies all events, one cell per lane; with 32 cells (eight threads per
// cell) wavefront w holds groups 2 w and 2 w + 1 and the owners are lanes 0-31 of wavefront 0.  (Cell-major — thread
// 4 c + q — left every wavefront walking the Kalman loop with one lane in four at work.)
//
// mupdate_body is the front every instantiation shares — round trip 1, the masks, the event numbers; its pieces are the
// functions mupd_* below — and then the owners' walk of its variant: mupd_walk_plain (no ray stage) or mupd_walk_ray
// (raycast_enabled).  A walk runs the rounds of the exchange (mupd_exchange, shared), applies the owner's events of each
// round and stores the cell.
//
// What the front hands the walk: the thread's place in the block, its cell and the batch's scans that concern it.
struct MCell {
  unsigned bid, cpb;        // the block | cells per block
  unsigned o, cl, cq;       // the cell in memory order | in the block | the thread's group of four scans
  unsigned count;           // scans of the batch
  bool owner;               // this thread applies the cell's events
  unsigned nib;             // bit j: scan 4 cq + j observed the cell
  unsigned base, total;     // the number of the thread's first event | the block's events
  unsigned tmask, smask;    // scans that observed the cell | whose move vacated it
  unsigned umask;           // scans that observed any cell
  unsigned rmask, runmask;  // ray stage (else 0): scans that left evidence or a ray height in the cell | whose stage runs
};

// Block 0 behind round trip 1: thread 0 commits the geometry ring behind the batch (make_ctx does this per scan), threads
// 64 .. 64 + kMaxBatch re-arm the state of the batch after next.
template <int CH, bool RAY>
__device__ __forceinline__ void mupd_commit(const MUpd& U, DevState* __restrict__ st, const unsigned bid, const unsigned count,
                                            MState* const ms, const unsigned passbits, const unsigned umask,
                                            const unsigned runmask) {
  constexpr bool has_int = (CH & 1) != 0, has_col = (CH & 2) != 0;
  const unsigned lt = threadIdx.x;
  if (bid == 0 && lt == 0) {
    const unsigned last = count - 1u;
    const unsigned slot_next = (U.scan_no0 + count) & 3u;
    DevGeom g = ms->E[last];
    const DevCand cl2 = ms->C[last];
    const bool applied_last = U.do_move && (!U.gate_on_filter || ((passbits >> last) & 1u) != 0u);
    if (applied_last) { g.px = cl2.px; g.py = cl2.py; g.sr = cl2.sr; g.sc = cl2.sc; }
    const unsigned ob_prev = st->obst[U.scan_no0 & 3u].scan;
    st->geom[slot_next] = g;
    st->cand[(U.scan_no0 + last) & 3u] = cl2;   // (the synchronous statistics report the last scan's shift)
    // the last scan of the batch that observed a cell (umask: one bit per scan)
    st->obst[slot_next].scan = umask ? U.scan_no0 + (31u - unsigned(__clz(int(umask)))) : ob_prev;
#pragma unroll
    for (int q = 0; q < 4; ++q) { st->flags[q].any_pass = 0u; st->flags[q].any_inside = 0u; st->flags[q].ray_any = 0u; }
    if (umask) {
      const unsigned first_upd = U.scan_no0 + unsigned(__ffs(int(umask))) - 1u;
      if (has_int && st->vis_int == 0u) st->vis_int = 3u * first_upd + 2u;
      if (has_col && st->vis_col == 0u) st->vis_col = 3u * first_upd + 2u;
    }
    if constexpr (RAY) {  // the three layers become visible with the first frame that runs (raycasting.cpp:223-226)
      if (runmask && st->vis_ray == 0u) st->vis_ray = 3u * (U.scan_no0 + unsigned(__ffs(int(runmask))) - 1u) + 3u;
    }
  }
  if (bid == 0 && lt >= 64u && lt < 64u + unsigned(kMaxBatch)) {
    U.rearm->inside[lt - 64u] = 0u;
    if (lt == 64u) { U.rearm->flags[0] = 0u; U.rearm->flags[1] = 0u; U.rearm->flags[2] = 0u; }
  }
}
// Which scans' moves vacated cell o (lane k holds scan k's geometry; stripmask: the scans whose move vacated any cell).
__device__ __forceinline__ unsigned mupd_vacated(unsigned stripmask, const GeomConst& G, const unsigned o, const bool valid,
                                                 const int v_sr, const int v_sc, const int v_shr, const int v_shc) {
  unsigned smask = 0u;
  const int r = int(o % unsigned(G.s_rows)) + G.s_r0;
  const int col = int(o / unsigned(G.s_rows)) + G.s_c0;
  while (stripmask) {
    const unsigned k = unsigned(__ffs(int(stripmask))) - 1u;
    stripmask &= stripmask - 1u;
    const int sr = __builtin_amdgcn_readlane(v_sr, int(k)), sc = __builtin_amdgcn_readlane(v_sc, int(k));
    const int shr = __builtin_amdgcn_readlane(v_shr, int(k)), shc = __builtin_amdgcn_readlane(v_shc, int(k));
    if (in_cleared_strip(r, sr, shr, G.rows) || in_cleared_strip(col, sc, shc, G.cols)) smask |= 1u << k;
  }
  if (!valid) smask = 0u;
  return smask;
}
// The block's (cell, scan) events, numbered cell-major / scan-minor: a cell's events stay one run, in scan order.  Lane
// c < cpb of EVERY wavefront holds cell c's mask, so each wavefront sums the cells in front for itself.  Returns the
// number of the thread's first event; total: the block's events.
__device__ __forceinline__ unsigned mupd_number(const unsigned tmask, const unsigned tpc, const unsigned cpb,
                                                const unsigned cl, const unsigned cq, unsigned& total) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned mine = lane < cpb ? unsigned(__popc(tmask)) : 0u;
  unsigned inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned v = __shfl_up(inc, d);
    if (int(lane) >= d) inc += v;
  }
  total = unsigned(__builtin_amdgcn_readlane(int(inc), 63));
  unsigned base = inc - mine;                                     // the events of the cells in front of this one,
  if (tpc == 8u) base = unsigned(__shfl(int(base), int(cl)));     // (lanes 32-63: a second group of the same 32 cells)
  base += unsigned(__popc(tmask & lowbits(unsigned(kScansPerThread) * cq)));  // the cell's own in earlier groups
  return base;
}
// One round [r0, r1) of the exchange: every thread lists its (at most four) events of the round, then round trip 2
// fetches {aux, zs, obs} of every listed event, spread evenly over the block (kEvCap / 256 per thread), leaves the
// observations in S.ob / S.rgb for the owners and the scratch clean.  `join`: what else leaves with round trip 2.
template <typename POLICY, int CH, typename LDS, typename JOIN>
__device__ __forceinline__ void mupd_exchange(const MUpd& U, const typename POLICY::Layers& L, LDS& S, const MCell& c,
                                              const unsigned long long (&kk)[kScansPerThread], const unsigned ncell,
                                              const unsigned r0, const unsigned r1, JOIN join) {
  constexpr bool has_int = (CH & 1) != 0, has_col = (CH & 2) != 0;
  const float nanv = __uint_as_float(0x7FC00000u);
  const unsigned lt = threadIdx.x, bid = c.bid, cpb = c.cpb;
  {
    unsigned e = c.base;
#pragma unroll
    for (int j = 0; j < kScansPerThread; ++j) {
      if ((c.nib >> j) & 1u) {
        if (e >= r0 && e < r1) {
          MEvent ev;
          ev.idx = uint32_t(kk[j]);
          ev.cell = uint16_t(c.cl);
          ev.k = uint16_t(c.cq * unsigned(kScansPerThread) + unsigned(j));
          S.ev[e - r0] = ev;
        }
        ++e;
      }
    }
  }
  __syncthreads();
  constexpr int kPer = kEvCap / 256;
  MEvent ev_[kPer];
  float2 ob_[kPer];
  uint4 ax_[kPer];
  uint2 zs_[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const unsigned j = lt + unsigned(q) * 256u;
    ob_[q] = make_float2(kFltMax, 0.0f);  // (no finite z: FLT_MAX, variance 0 — elevation_mapping.hpp:26-34)
    ax_[q] = make_uint4(0u, 0u, 0u, 0u);
    zs_[q] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    ev_[q].idx = kNoIdx; ev_[q].cell = 0; ev_[q].k = 0;
    if (r0 + j < r1) {
      ev_[q] = S.ev[j];
      const size_t oc = size_t(ev_[q].k) * ncell + (bid * cpb + ev_[q].cell);
      if (ev_[q].idx != kNoIdx) ob_[q] = U.obs[size_t(ev_[q].k) * U.obs_stride + ev_[q].idx];
      ax_[q] = U.aux[oc];
      zs_[q] = U.zs[oc];
    }
  }
  join();
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const unsigned j = lt + unsigned(q) * 256u;
    if (r0 + j >= r1) continue;
    if (has_col) S.rgb[j] = U.cobs[size_t(ev_[q].k) * U.obs_stride + ax_[q].w];  // (one more dependent gather)
    const uint32_t zm = ax_[q].x, imx = ax_[q].y, fst = ~ax_[q].z;  // (the scratch holds ~fst: mbin_body's flush)
    MObs ob;
    ob.min_z = ob_[q].x;
    ob.var = POLICY::obs_var(L, ob_[q].y);  // (Kalman: R, substituted here by 256 threads and not in the owners' walk)
    // (a zero maximum takes the sign of the first zero-valued point, see Scratch::zs)
    ob.max_z = zm ? ((zm == 0x80000000u && (zs_[q].x & 1u)) ? -0.0f : unord(zm)) : -kFltMax;
    ob.iobs = 0.0f;
    if (has_int) ob.iobs = (fst & 1u) ? nanv : ((imx == 0x80000000u && (zs_[q].y & 1u)) ? -0.0f : unord(imx));
    S.ob[j] = ob;
    FDM_PHASE(1);  // round trip 2 (observations, record) back
    const size_t oc = size_t(ev_[q].k) * ncell + (bid * cpb + ev_[q].cell);
    U.key[oc] = kEmptyKey;  // the scratch is clean again for the batch after next
    U.aux[oc] = make_uint4(0u, 0u, 0u, 0u);
    if ((zs_[q].x & zs_[q].y) != 0xFFFFFFFFu) U.zs[oc] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
  }
}
// NaN in layers [from, to) of cell o, eight at a time: eight pointers from `layer(l)`, then eight stores through CELL*
// (float, or float in address space 1: global memory, no flat store).
template <typename CELL, typename SRC>
__device__ __forceinline__ void mwipe_layers(const int from, const int to, const unsigned o, SRC layer) {
  const float nanv = __uint_as_float(0x7FC00000u);
  for (int l0 = from; l0 < to; l0 += 8) {
    float* p[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) p[q] = layer(l0 + q);
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (l0 + q < to) ((CELL*)p[q])[o] = nanv;
  }
}

// ---- the owners' walk without the ray stage ----
// It is the launch's longest dependent chain — ONE wavefront issuing in order, as long as (events of the block's busiest
// cell) x (instructions per event) — so everything an event does not change is decided here, once.  An owner knows its
// cell's scans (tmask) and the scans whose move vacated it (smask): the cell is wiped in front of its event of ordinal i
// exactly when some vacating scan s has that event as the first one at or after s (scan s moves the map BEFORE it
// observes: an event of scan s itself counts) — bit 31 - i of `wrev`, tested by sign and shifted out per event; a
// vacating scan behind the last event wipes in the tail (wipe_tail).  No flags travel through the loop: an event happened
// / the record and the obstacle cell are dirty <=> tmask != 0 (a wipe inside the walk is always followed by an event),
// some strip wiped the cell <=> wrev != 0 || wipe_tail.
template <typename POLICY, int CH>
__device__ __forceinline__ void mupd_walk_plain(const MUpd& U, const typename POLICY::Layers& L,
                                                MUpdLds<(CH & 2) != 0, false>& S, const MCell& c,
                                                const unsigned long long (&kk)[kScansPerThread], const unsigned ncell,
                                                float* const* __restrict__ all_layers, const int n_layers) {
  constexpr bool has_int = (CH & 1) != 0, has_col = (CH & 2) != 0;
  const float nanv = __uint_as_float(0x7FC00000u);
  const unsigned o = c.o;
  typename POLICY::State stt;
  POLICY::set_nan(stt);
  float sint = nanv;
  unsigned e_next = c.base;        // the number of the owner's next event
  uint32_t colv = 0x7FC00000u;
  unsigned wrev = 0u, left = 0u;   // left: the owner's events still to be applied
  const typename POLICY::WalkRegs wregs = POLICY::walk_regs(L);
  bool wipe_tail = false, strip_walk = false;
  float zlo = 0.0f, zhi = 0.0f;    // min_z / max_z of the cell's last observation (the obstacle layer reads only that one)
  if (c.owner) {
    left = unsigned(__popc(c.tmask));
    unsigned wbefore = 0u;
    for (unsigned sm = c.smask; sm; sm &= sm - 1u) {
      const unsigned s = unsigned(__ffs(int(sm))) - 1u;       // (< count <= 32)
      const unsigned at = c.tmask & ~((1u << s) - 1u);         // the cell's events of scans >= s
      if (at) wbefore |= 1u << unsigned(__popc(c.tmask & ((1u << (unsigned(__ffs(int(at))) - 1u)) - 1u)));
      else wipe_tail = true;
    }
    wrev = __brev(wbefore);
    strip_walk = wbefore != 0u;
  }
#pragma unroll 1
  for (unsigned r0 = 0; r0 < c.total; r0 += unsigned(kEvCap)) {  // one round for all but the densest corners
    const unsigned r1 = min(r0 + unsigned(kEvCap), c.total);
    mupd_exchange<POLICY, CH>(U, L, S, c, kk, ncell, r0, r1, [&]() {
      if (r0 == 0u && c.owner && c.tmask) {  // (the record joins the same round trip)
        POLICY::load(L, o, stt);
        if (has_int) sint = L.intensity[size_t(o) * L.istride];
      }
    });
    __syncthreads();
    // The owner's events of this round are one run of the list, known before the round: counted down, the
    // observation of event i + 1 read from LDS before the arithmetic of event i.  No scan number in the loop (the
    // wipes go by event ordinal, see wrev); the obstacle value and the colour are the last event's, taken behind it.
    unsigned n = (left != 0u && e_next < r1) ? min(left, r1 - e_next) : 0u;  // (left != 0: e_next >= r0)
    if (n) {
      const MObs* p = &S.ob[e_next - r0];
      e_next += n;
      left -= n;
      auto apply = [&](const MObs& ob) {
        const bool fresh = int(wrev) < 0;  // vacated since the last event: NaN in every layer (GridMap::move)
        wrev <<= 1;
        POLICY::walk_step(L, wregs, stt, ob.min_z, ob.var, ob.max_z, fresh);
        if (has_int) {  // isnan(sint) || iobs > sint, two-sided (iobs can be NaN: a NaN intensity as the cell's first point)
          const float hi = (ob.iobs > sint) ? ob.iobs : sint;
          const float hn = isnan(sint) ? ob.iobs : hi;
          sint = fresh ? ob.iobs : hn;
        }
      };
      MObs nx = *p;
      while (--n) {
        const MObs ob = nx;
        nx = *++p;
        __builtin_amdgcn_sched_barrier(0);  // (the read stays in front of the arithmetic: its latency is the loop's otherwise)
        apply(ob);
      }
      apply(nx);
      zlo = nx.min_z; zhi = nx.max_z;
      if (has_col) colv = S.rgb[p - S.ob] & 0x00FFFFFFu;  // (a later round's last event overwrites it)
    }
    __syncthreads();  // (the next round reuses the lists)
  }
  FDM_PHASE(2);  // events applied
  // The tail behind the walk, still on the launch's longest chain: every value the owner stores is computed first —
  // the sample variance and the bounds included — then the stores leave back to back, in the order they always had
  // (all-layer NaN, the record's NaN, record, obstacle, intensity, colour: a lane's stores to one address stay in
  // program order, which is all the order there is to keep), with no load from global memory and no wait between them.
  if (c.owner) {
    const bool any_evt = c.tmask != 0u;
    const unsigned last1 = 32u - unsigned(__clz(int(c.tmask)));  // the last event's scan + 1 (no event: 0)
    const bool strips = strip_walk || wipe_tail;
    // map_.clear(obstacle) by every scan that observed a cell (elevation_mapping.cpp:144-146), behind the cell's last observation
    const bool obst_clear = wipe_tail || (c.umask & lowbits(c.count) & ~lowbits(last1)) != 0u;
    const float obst_v = (any_evt && !obst_clear && zhi > zlo) ? zhi : nanv;
    if (wipe_tail) { sint = nanv; colv = 0x7FC00000u; }  // vacated behind the last event: the wipe is all that is stored
    POLICY::finish(stt);  // (no event: of a NaN state, not stored)
    POLICY::settle(stt);
    if (strips) {  // the pointers from the LDS table; beyond what it holds, from memory
      using gfloat = __attribute__((address_space(1))) float;  // (layers are global memory: no flat store)
      static_assert(kLayTab % 8 == 0, "the wipe reads the table in groups of eight");
      mwipe_layers<gfloat>(0, min(n_layers, kLayTab), o, [&](int l) { return S.lay[l]; });
      mwipe_layers<gfloat>(kLayTab, n_layers, o, [&](int l) { return all_layers[min(l, n_layers - 1)]; });
      POLICY::clear_cell(L, o);
    }
    if (any_evt && !wipe_tail) POLICY::store(L, o, stt);
    if (any_evt || obst_clear) L.obstacle[o] = obst_v;
    if (has_int && (any_evt || strips)) L.intensity[size_t(o) * L.istride] = sint;
    if (has_col && (any_evt || strips)) reinterpret_cast<uint32_t*>(L.color)[o] = colv;
  }
}

// ---- the owners' walk with the ray stage ----
// Rays cross most cells of the map, so nearly every cell has an event and the cell's stored state was asked for with
// round trip 1 (MRayEarly).  The walk goes by scan number over the cell's observations (m) and ray events (rm) together
// and resolves scan k's raycasting stage behind scan k's observation.  (These instantiations have no register to spare:
// loop and tail are the ones the update half had before the walk above was shortened.)
template <typename POLICY>
struct MRayEarly {  // the owner's record, intensity and visibility log-odds as stored
  typename POLICY::State rec;
  float sint, lo;
};
template <typename POLICY, int CH>
__device__ __forceinline__ void mupd_walk_ray(const MUpd& U, const typename POLICY::Layers& L,
                                              MUpdLds<(CH & 2) != 0, true>& S, const MCell& c,
                                              const unsigned long long (&kk)[kScansPerThread], const unsigned ncell,
                                              float* const* __restrict__ all_layers, const int n_layers,
                                              const MRayEarly<POLICY>& early) {
  constexpr bool has_int = (CH & 1) != 0, has_col = (CH & 2) != 0;
  const float nanv = __uint_as_float(0x7FC00000u);
  const unsigned o = c.o, cl = c.cl;
  const MRay& ray = U.ray;
  typename POLICY::State stt;
  POLICY::set_nan(stt);
  float sint = nanv;
  unsigned lastp1 = 0u, m = c.owner ? c.tmask : 0u, e_next = c.base;  // (owner: the events still to be applied, the next one's number)
  unsigned rm = c.owner ? c.rmask : 0u;                                // ... and its ray events
  unsigned lastu1 = 0u;                                                // (behind the cell's last OBSERVATION; lastp1 counts ray events too)
  bool evt = false, st_dirty = false, strip_any = false, obst_dirty = false;
  float obst = nanv;
  uint32_t colv = 0x7FC00000u;
  // raycasting state of the cell: visibility log-odds, the elevation the last event left, what the raycasting layer ends
  // up with (the LAST running frame's minimum: map.clear(raycasting) + that frame's rays)
  float lo = nanv, elev = nanv, ray_val = nanv;
  bool lo_dirty = false, ghost_one = false;
  const int k_last_run = c.runmask ? 31 - __clz(int(c.runmask)) : -1;
  // NaN in every layer of the cell: a strip GridMap::move vacated, or ElevationMap::clearAt (elevation_map.hpp:131-135)
  auto wipe = [&]() {
    POLICY::set_nan(stt);
    sint = nanv;
    colv = 0x7FC00000u;
    strip_any = true;
    st_dirty = false;
    obst = nanv; obst_dirty = true; lo = nanv; lo_dirty = false; ghost_one = false; elev = nanv; ray_val = nanv;
  };
  // resolveGhostCells (raycasting.cpp:175-202) for this cell and scan k: the scan's evidence, then its ghost decision
  auto resolve = [&](const unsigned k) {
    const uint32_t cnt = S.rcnt[k * kUpdCells + cl], hmin = S.rmin[k * kUpdCells + cl];
    if (cnt) {  // observed evidence, once per ray-scan point in the cell (raycasting.cpp:156-163)
      if (isnan(lo)) lo = 0.0f;
      for (uint32_t q = 0; q < cnt; ++q) {
        const float a = lo + ray.l_obs;
        const float nx = (ray.l_max < a) ? ray.l_max : a;  // std::min(a, l_max)
        if (nx == lo) break;  // fixed point reached: the remaining folds change nothing
        lo = nx;
      }
      lo_dirty = true;
    }
    float rv = nanv;
    if (hmin != kMRayEmpty) {
      rv = unord(hmin);
      if (!isnan(elev) && elev > rv + ray.conflict_thr) {
        if (isnan(lo)) lo = 0.0f;
        lo -= ray.l_ghost;
        lo_dirty = true;
        if (lo < ray.clear_thr) {  // clearAt: NaN in every layer, then the marker (no min ray height for the frame)
          wipe();
          ghost_one = true;
          rv = nanv;
        }
      }
    }
    if (int(k) == k_last_run) ray_val = rv;
  };
  if (c.owner) {
    if (c.tmask | c.rmask) {
      stt = early.rec;
      if (has_int) sint = early.sint;
      elev = POLICY::elevation(stt);
      if (c.rmask) lo = early.lo;
    }
  }
#pragma unroll 1
  for (unsigned r0 = 0; r0 < c.total; r0 += unsigned(kEvCap)) {  // one round for all but the densest corners
    const unsigned r1 = min(r0 + unsigned(kEvCap), c.total);
    mupd_exchange<POLICY, CH>(U, L, S, c, kk, ncell, r0, r1, []() {});
    __syncthreads();
    // the cells' own threads apply their events of this round, in scan order
    while (m | rm) {
      const unsigned k = unsigned(__ffs(int(m | rm))) - 1u, bit = 1u << k;
      if ((m & bit) && e_next >= r1) break;  // (its observation arrives with the next round)
      const unsigned upto = lowbits(k + 1u), from = lowbits(lastp1);  // scans lastp1 .. k
      if (c.smask & upto & ~from) wipe();  // vacated since the last event: NaN in every layer (GridMap::move)
      if (m & bit) {
        m &= ~bit;
        const MObs ob = S.ob[e_next - r0];
        const uint32_t rgb = has_col ? S.rgb[e_next - r0] : 0u;
        ++e_next;
        POLICY::step(L, stt, ob.min_z, ob.var, ob.max_z);
        obst = (ob.max_z > ob.min_z) ? ob.max_z : nanv;
        obst_dirty = true;
        if (has_int && (isnan(sint) || ob.iobs > sint)) sint = ob.iobs;
        if (has_col) colv = rgb & 0x00FFFFFFu;
        evt = true;
        st_dirty = true;
        elev = POLICY::elevation(stt);
        lastu1 = k + 1u;
      }
      if (rm & bit) {  // scan k's raycasting stage, behind its observation
        rm &= ~bit;
        resolve(k);
      }
      lastp1 = k + 1u;
    }
    __syncthreads();  // (the next round reuses the lists)
  }
  while (rm) {  // ray events behind the block's last observation (or of a block without any)
    const unsigned k = unsigned(__ffs(int(rm))) - 1u;
    rm &= rm - 1u;
    const unsigned upto = lowbits(k + 1u), from = lowbits(lastp1);
    if (c.smask & upto & ~from) wipe();
    resolve(k);
    lastp1 = k + 1u;
  }
  FDM_PHASE(2);  // events applied
  if (c.owner) {  // the scans after the cell's last event, then the stores
    const unsigned all = lowbits(c.count), from = lowbits(lastp1);
    if (c.smask & all & ~from) {
      strip_any = true; st_dirty = false; sint = nanv; colv = 0x7FC00000u; obst = nanv; obst_dirty = true;
      lo = nanv; lo_dirty = false; ghost_one = false; ray_val = nanv;
    }
    // map_.clear(obstacle) by every scan that observed a cell (elevation_mapping.cpp:144-146), behind the cell's last observation
    if (c.umask & all & ~lowbits(lastu1)) { obst = nanv; obst_dirty = true; }
    if (strip_any) {
      mwipe_layers<float>(0, n_layers, o, [&](int l) { return all_layers[min(l, n_layers - 1)]; });
      POLICY::clear_cell(L, o);
    }
    if (st_dirty) {
      POLICY::finish(stt);
      POLICY::store(L, o, stt);
    }
    if (obst_dirty) L.obstacle[o] = obst;
    if (has_int && (evt || strip_any)) L.intensity[size_t(o) * L.istride] = sint;
    if (has_col && (evt || strip_any)) reinterpret_cast<uint32_t*>(L.color)[o] = colv;
    if (ray.stamp) {
      if (lo_dirty) ray.logodds[o] = lo;
      if (ghost_one) ray.ghost[o] = 1.0f;
      if (c.runmask) ray.ray_min[o] = ray_val;  // every cell, every running frame: the layer is cleared first (raycasting.cpp:228)
    }
  }
}

template <typename POLICY, int CH, bool RAY>
__device__ __forceinline__ void mupdate_body(const MUpd& U_, const GeomConst& G_, DevState* __restrict__ st,
                                             const typename POLICY::Layers& L_,
                                             float* const* __restrict__ all_layers, int n_layers,
                                             const unsigned ncell, const unsigned bid, const unsigned count,
                                             const unsigned long long* const u_key, MState* const u_ms,
                                             MUpdLds<(CH & 2) != 0, RAY>& S) {
  // (count, U.key and U.ms arrive with the kernel's head: the key loads and the geometry loads wait for nothing else)
  const MUpd& U = U_;
  const GeomConst& G = G_;
  const typename POLICY::Layers& L = L_;
  const unsigned lt = threadIdx.x, lane = lt & 63u, wave = lt >> 6;
  const unsigned tpc = upd_threads_per_cell(count), cpb = 256u / tpc;   // threads per cell, cells per block (block-uniform)
  const unsigned cl = lt & (cpb - 1u), cq = tpc == 8u ? lt >> 5 : lt >> 6;   // cell of the block, group of four scans
  const unsigned o = bid * cpb + cl;
  const bool valid = o < ncell;
  const bool owner = valid && cq == 0u;  // the thread that applies the cell's events: wavefront 0, lane = cell
  MState* const ms = u_ms;

  // ---- round trip 1: the thread's four keys, the per-scan geometry (lane j holds scan j's) ----
  unsigned long long kk[kScansPerThread];
#pragma unroll
  for (int j = 0; j < kScansPerThread; ++j) {
    const unsigned k = cq * unsigned(kScansPerThread) + unsigned(j);
    kk[j] = kEmptyKey;
    if (k < count && valid) kk[j] = u_key[size_t(k) * ncell + o];
  }
  float* lay_p = nullptr;  // (wavefront 1, no owner in it: the layer pointers join round trip 1)
  if constexpr (!RAY) {
    if (wave == 1u && int(lane) < min(n_layers, kLayTab)) lay_p = all_layers[lane];
  }
  int v_sr = 0, v_sc = 0, v_shr = 0, v_shc = 0;
  unsigned v_in = 0u;
  bool v_run = false;
  if (lane < count) {
    v_sr = ms->E[lane].sr; v_sc = ms->E[lane].sc;
    v_shr = ms->C[lane].shr; v_shc = ms->C[lane].shc;
    v_in = ms->inside[lane];
    if constexpr (RAY) {
      if (U.ray.stamp) v_run = U.ray.rs->any[lane] == U.ray.stamp && U.ray.rs->origin_in[lane] != 0u;
    }
  }
  // raycasting: the thread's four (evidence count, min ray height) pairs join round trip 1 (the images of a scan whose
  // stage did not run are clean: no events) ... and so does the cell's stored state: with raycasting nearly every cell has
  // an event, and asking for the record only once the images are back would be one more dependent round trip
  uint32_t rc_[kScansPerThread], rh_[kScansPerThread];
  MRayEarly<POLICY> early;
  unsigned runmask = 0u;  // scans whose raycasting stage runs (raycasting.cpp:207-220)
  if constexpr (RAY) {
#pragma unroll
    for (int j = 0; j < kScansPerThread; ++j) {
      const unsigned k = cq * unsigned(kScansPerThread) + unsigned(j);
      rc_[j] = 0u; rh_[j] = kMRayEmpty;
      if (U.ray.stamp && k < count && valid) {
        rc_[j] = U.ray.rc_cnt[size_t(k) * ncell + o];
        rh_[j] = U.ray.rc_min[size_t(k) * ncell + o];
      }
    }
    POLICY::set_nan(early.rec);
    early.sint = early.lo = __uint_as_float(0x7FC00000u);
    if (owner) {
      POLICY::load(L, o, early.rec);
      if ((CH & 1) != 0) early.sint = L.intensity[size_t(o) * L.istride];
      if (U.ray.stamp) early.lo = U.ray.logodds[o];
    }
    runmask = uni(unsigned(__ballot(v_run)));
  }
  const unsigned passbits = uni(ms->flags[0]);
  const bool v_applied = lane < count && U.do_move && (!U.gate_on_filter || ((passbits >> lane) & 1u) != 0u);
  const unsigned umask = uni(unsigned(__ballot(lane < count && v_in != 0u)));                     // scans that observed a cell
  const unsigned stripmask = uni(unsigned(__ballot(v_applied && (v_shr != 0 || v_shc != 0))));   // scans whose move vacated cells

  mupd_commit<CH, RAY>(U, st, bid, count, ms, passbits, umask, runmask);

  unsigned nib = 0u;
#pragma unroll
  for (int j = 0; j < kScansPerThread; ++j) nib |= (kk[j] != kEmptyKey) ? (1u << j) : 0u;
  FDM_PHASE(0);  // round trip 1 (keys, geometry) back
  // the cell's scans: the threads of a cell sit in different wavefronts, their parts meet in LDS (lt == cq * cpb + cl)
  S.mk.tpart[lt] = nib << (unsigned(kScansPerThread) * cq);
  if constexpr (!RAY) {
    if (wave == 1u) S.lay[lane] = lay_p;  // (all kLayTab entries: null beyond n_layers, read but never stored through)
  }
  if constexpr (RAY) {
    unsigned rb = 0u;
#pragma unroll
    for (int j = 0; j < kScansPerThread; ++j) {
      const unsigned k = cq * unsigned(kScansPerThread) + unsigned(j);
      if (rc_[j] != 0u || rh_[j] != kMRayEmpty) {
        rb |= 1u << j;
        if (rc_[j] != 0u) U.ray.rc_cnt[size_t(k) * ncell + o] = 0u;  // the images are clean again for the next batch
        if (rh_[j] != kMRayEmpty) U.ray.rc_min[size_t(k) * ncell + o] = kMRayEmpty;
      }
      S.rcnt[k * kUpdCells + cl] = rc_[j];
      S.rmin[k * kUpdCells + cl] = rh_[j];
    }
    S.mk.rpart[lt] = rb << (unsigned(kScansPerThread) * cq);
  }
  // which scans' moves vacated THIS cell (asked by the owners only)
  unsigned smask = 0u;
  if (stripmask && cq == 0u) smask = mupd_vacated(stripmask, G, o, valid, v_sr, v_sc, v_shr, v_shc);

  __syncthreads();
  unsigned tmask = 0u, rmask = 0u;  // the cell's scans | its ray events: scans whose stage left evidence or a ray height in it
#pragma unroll
  for (unsigned g = 0; g < 4u; ++g) tmask |= S.mk.tpart[g * cpb + cl];
  if (tpc == 8u) {
#pragma unroll
    for (unsigned g = 4; g < 8u; ++g) tmask |= S.mk.tpart[g * cpb + cl];
  }
  if constexpr (RAY) {
    if (cq == 0u)
      for (unsigned g = 0; g < tpc; ++g) rmask |= S.mk.rpart[g * cpb + cl];
  }
  unsigned total;
  const unsigned base = mupd_number(tmask, tpc, cpb, cl, cq, total);

  const MCell c{bid, cpb, o, cl, cq, count, owner, nib, base, total, tmask, smask, umask, rmask, runmask};
  if constexpr (RAY) mupd_walk_ray<POLICY, CH>(U, L, S, c, kk, ncell, all_layers, n_layers, early);
  else mupd_walk_plain<POLICY, CH>(U, L, S, c, kk, ncell, all_layers, n_layers);
  // touched-cell count of the batch's last scan (what the synchronous statistics report), per update block
  const unsigned long long mt = __ballot(owner && ((tmask >> (count - 1u)) & 1u) != 0u);
  if (lane == 0u) S.s_t[wave] = unsigned(__popcll(mt));
  __syncthreads();
  if (lt == 0 && bid * cpb < ncell) U.upd_part[bid] = S.s_t[0] + S.s_t[1] + S.s_t[2] + S.s_t[3];
}

// [ update of batch b-1 | bin of batch b | crop pass of batch b+1 ] — any of the three may be empty.
// Grid: blockIdx.x = block inside a scan (as wide as the widest scan of the two halves); blockIdx.y = first
// `upd_rows` rows of update blocks (block = row * width + x), then one row per scan of the bin half, then one row per
// scan of the crop half.  Surplus blocks leave at once.  Rows are dispatched in order: the update's chains first.
// (the P2 estimator's 17-float state does not fit the 80 registers of 6 waves per SIMD without spilling: 5 there)
template <typename POLICY> struct MBatchWaves { static constexpr int value = FDM_MB_WAVES; };
template <> struct MBatchWaves<P2RecPolicy> { static constexpr int value = FDM_MB_WAVES - 1; };
template <> struct MBatchWaves<P2Policy> { static constexpr int value = FDM_MB_WAVES - 1; };

// The HEAD: the eight leading scalars are everything that decides which half a block belongs to and which scan or cells
// are its own — the launch geometry (with the grid's width, so the hidden gridDim.x is not read), the three halves' scan
// counts (copies of U.count, B.count, Cn.count) and whether stamps are wanted — and directly behind them lie the two
// pointers an update block's first loads go through (MUpd::key, MUpd::ms).  They are fetched in one batch and used
// unconditionally: one scalar round trip, then a bin or scout block fetches its scan's record (a second one) and its
// vector loads leave.  The parent's arguments were a chain of dependent reads 5-8 deep (timeline pointer -> upd_rows ->
// B.count -> n[k] -> px[k] ... -> ms -> prev -> prev_count), about 0.2 us each under this launch
// (scripts/ubench/kernarg_chain.hip).  t0 is taken without waiting for an argument.
template <typename POLICY, int CH, bool RAY>
__global__ __launch_bounds__(256, MBatchWaves<POLICY>::value) void k_mbatch(unsigned upd_rows, unsigned n_upd_blocks, unsigned ncell,
                                                unsigned width, unsigned u_count, unsigned b_count, unsigned c_count,
                                                unsigned stamps, unsigned long long* u_key, MState* u_ms,
                                                const MUpd U, const MBin B, const MCrop Cn,
                                                const MCommon K, const GeomConst G, DevState* __restrict__ st,
                                                const typename POLICY::Layers L,
                                                float* const* __restrict__ all_layers, int n_layers) {
  __shared__ __align__(16) unsigned char lds[kMLdsBytes<(CH & 2) != 0, RAY>];
  const unsigned long long t0 = wall_clock64();
  FDM_SGPR_NOW10(upd_rows, n_upd_blocks, ncell, width, u_count, b_count, c_count, stamps, u_key, u_ms);
#if FDM_MB_PHASES
  if (threadIdx.x == 0) { g_phase[0] = g_phase[1] = g_phase[2] = unsigned(t0); }
#endif
  const unsigned row = blockIdx.y, x = blockIdx.x;
  if (row < upd_rows) {
    const unsigned ub = row * width + x;
    if (ub < n_upd_blocks)
      mupdate_body<POLICY, CH, RAY>(U, G, st, L, all_layers, n_layers, ncell, ub, u_count, u_key, u_ms,
                                    *reinterpret_cast<MUpdLds<(CH & 2) != 0, RAY>*>(lds));
  } else if (row < upd_rows + b_count) {  // (a surplus block of a short row leaves inside, behind its record)
    mbin_body<CH, RAY>(B, K, G, st, ncell, row - upd_rows, x, *reinterpret_cast<MBinLds*>(lds));
  } else {  // scout rows: block c of c_count * kMScout
    const unsigned c = (row - upd_rows - b_count) * width + x;
    if (c < c_count * kMScout) mcrop_body(Cn, K, c / kMScout, c % kMScout);
    else if (c == c_count * kMScout && c_count) mwalk_body(B, Cn, K, G, st, b_count, c_count);
  }
  if (stamps && threadIdx.x == 0) {  // (thread 0's view of the block; scripts/timeline_batch.py)
    const unsigned b = blockIdx.y * width + x;
    K.timeline[2u * b] = t0;
#if FDM_MB_PHASES
    K.timeline[2u * b + 1u] = phase_word(t0);
#else
    K.timeline[2u * b + 1u] = wall_clock64();
#endif
  }
}

}  // namespace fdm
