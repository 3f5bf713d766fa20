"""The large cases of the segmentation tests, beside tests/seg_cases.py so that the small table stays fast: lists long
enough, and cell boxes wide enough, to reach the branches of fastdem_amd/csrc/fdm_segment.hpp and fdm_engine_segment.inl
that only size reaches.  tests/test_seg_restate.py admits every case on the CPU and shows that the TRUNCATED computation
(the branch skipped) gives another answer; tests/test_segment_gpu.py compares the engine with the full one.

The thresholds, with the kernel and the constant each comes from — when a cap moves, the case named here moves with it:
  PLANE_COUNT_SWEEP  k_plane_count: launch_plane_count caps the grid at 2048 blocks of kSegTile = 1024 positions; a list
                     of one position more makes block 0 walk a second tile                       -> count_*
  PLANE_SUM_SWEEP    k_plane_sum<false / true>: seg_sum_blocks caps at kSegSumBlocks = 256 blocks of 256 lanes; one
                     inlier more gives a lane of the fixed tree a second term                    -> sum_*
  INDEX_CHECK_SWEEP  k_seg_index_check: its grid is capped at 2048 blocks of 256 (plane and cluster entries); an entry
                     past it is read by the strided loop only                                    -> index_check_stride()
  SCAN_CHUNK         k_pack_scan scans 1024 block counts per step, a block counts 256 positions: past 262 144 positions
                     the carry between steps is used (Compactor::run, k_seg_head_count / k_seg_heads / seg_run_of)
                                                                                                 -> ground_600k
  RS_SMALL_MAX       fdm_rsort.hpp: rs_tile(n) is 1024 pairs up to kRsSmallMax = 600 000, 4096 above (SortBufs64 and
                     SortBufs through rs_enqueue)                                                -> ground_600k
(The wide cell boxes — bits_x + bits_y above 32 in k_seg_pack_keys and the second sort — are small clouds: they are in
tests/seg_cases.py's table, ground_wide_*.)"""
import functools

import numpy as np

import seg_cases as SC
import seg_restate as SR

F = np.float32
PLANE_COUNT_SWEEP = 2048 * 1024
PLANE_SUM_SWEEP = 256 * 256
INDEX_CHECK_SWEEP = 2048 * 256
SCAN_CHUNK = 1024 * 256
RS_SMALL_MAX = 600000
ORDERS = tuple((o, s) for o in ("forward", "reversed", "pairwise") for s in ("eigh", "jacobi"))


# ------------------------------------------------------------------ the refinement's fixed tree ----
@functools.lru_cache(maxsize=None)
def sum_cases():
    """name -> (cloud, keyword arguments of segment_plane): tilted noisy planes of scene()'s construction whose inlier
    count is past PLANE_SUM_SWEEP — by at most 256, so that ONE partial block (block 0) takes a second term, and by far."""
    return {
        "sum_one_block": (SC.scene(6553, 130600, 0.5), dict(distance_threshold=0.05)),
        "sum_100k": (SC.scene(1000, 199000, 0.5), dict(distance_threshold=0.05)),
    }


# ------------------------------------------------------------------ the scoring kernel's second sweep ----
PLANE_A, PLANE_B = (0.05, -0.03, 0.4), (-0.2, 0.1, 3.0)
COUNT_TAIL = 400007  # (chosen so that the loop's 128 triplets hold one of plane A alone: see first_sweep_winner)


@functools.lru_cache(maxsize=None)
def count_base():
    """The cloud the long lists index: 90 000 points within +-0.005 of plane A, 90 000 of plane B, 120 000 uniform in
    the box of +-10.  (The noise is a tenth of the threshold: a model sampled from three points of a plane holds nearly
    all of that plane, so the larger plane wins whichever of its triplets comes first.)"""
    rng = np.random.default_rng(2097)
    parts = []
    for a, b, c in (PLANE_A, PLANE_B):
        px, py = rng.uniform(-10, 10, 90000), rng.uniform(-10, 10, 90000)
        parts.append(np.stack([px, py, a * px + b * py + c + rng.uniform(-0.005, 0.005, 90000)], axis=1))
    parts.append(rng.uniform(-10, 10, (120000, 3)))
    return SC._xyz(np.concatenate(parts))


@functools.lru_cache(maxsize=None)
def count_lists():
    """(head, one, tail): the first PLANE_COUNT_SWEEP list entries — 600 000 of plane A, 350 000 of plane B, the rest
    uniform, shuffled; duplicates throughout — the single entry of the T = 1 variant, and a tail of COUNT_TAIL entries of
    plane B alone: in the head plane A is the larger one, in head + tail plane B is.  (The tail's LENGTH sets the
    triplets the loop draws; with 400 000 none of the first 128 lay in plane A alone, and the winner was a triplet of
    plane B with or without the tail: that list could not fail for a skipped sweep.)"""
    rng = np.random.default_rng(2098)
    head = np.concatenate([rng.integers(0, 90000, 600000), rng.integers(90000, 180000, 350000),
                           rng.integers(180000, 300000, PLANE_COUNT_SWEEP - 950000)])
    head = head[rng.permutation(head.size)].astype(np.uint32)
    tail = rng.integers(90000, 180000, COUNT_TAIL).astype(np.uint32)
    return head, np.array([4242], dtype=np.uint32), tail


COUNT_KW = dict(distance_threshold=0.05, max_iterations=128)  # one batch of 128, run to the cap: both halves of the kernel


@functools.lru_cache(maxsize=None)
def count_cases():
    """name -> (cloud, keyword arguments of segment_plane).  *_list: the index list into count_base(); *_cloud: the
    same points in the same order as a plain cloud (the coalesced path), so that the two share their loop."""
    base = count_base()
    head, one, tail = count_lists()
    out = {}
    for name, extra in (("count_t1", one), ("count_tail", tail)):
        idx = np.concatenate([head, extra])
        out[name + "_list"] = (base, dict(COUNT_KW, indices=idx))
        out[name + "_cloud"] = (tuple(np.ascontiguousarray(v[idx]) for v in base), dict(COUNT_KW))
    return out


@functools.lru_cache(maxsize=None)
def count_loop(name):
    """The restatement's loop of a count case; "head": of the first PLANE_COUNT_SWEEP entries alone (both variants
    share them).  A *_cloud case takes its *_list case's loop: the listed points are the same."""
    base = count_base()
    if name == "head":
        return SR.ransac_loop(*base, indices=count_lists()[0], **COUNT_KW)
    if name.endswith("_cloud"):
        cloud, _ = count_cases()[name]
        loop = dict(count_loop(name[:-len("_cloud")] + "_list"))
        loop.update(cloud=cloud, indices=np.arange(cloud[0].size, dtype=np.uint32))
        return loop
    return SR.ransac_loop(*base, **count_cases()[name][1])


def plane_cases():
    return {**sum_cases(), **count_cases()}


@functools.lru_cache(maxsize=None)
def plane_loop(name):
    if name in count_cases():
        return count_loop(name)
    cloud, kw = sum_cases()[name]
    return SR.ransac_loop(*cloud, **kw)


@functools.lru_cache(maxsize=None)
def plane_answer(name, order="forward", solver="eigh"):
    return SR.finish_plane(plane_loop(name), order=order, solver=solver)


def first_sweep_winner(name):
    """(the loop's winning pass, the pass that wins if every hypothesis is scored against the first PLANE_COUNT_SWEEP list
    positions alone): the loop's own triplets and models, k_plane_count without its second sweep.  For loops that run to
    the cap (no early stop either way)."""
    loop = plane_loop(name)
    lx, ly, lz = (v[loop["indices"]] for v in loop["cloud"])
    full = loop["counts"].index(loop["best_count"])
    best, winner = 0, -1
    for j, (i1, i2, i3) in enumerate(SR.triplets(loop["indices"].size, loop["loop_iterations"])):
        model, valid = SR.plane_from_points(*[(lx[i], ly[i], lz[i]) for i in (i1, i2, i3)])
        assert int(valid) == loop["valid"][j]
        if not valid:
            continue
        cut = PLANE_COUNT_SWEEP
        count = int(np.count_nonzero(SR.plane_dist(model, lx[:cut], ly[:cut], lz[:cut]) < loop["threshold"]))
        if count > best:
            best, winner = count, j
    return full, winner


def first_collect(name):
    """The inlier list the refinement sums over: collectInliers with the unrefined model."""
    loop = plane_loop(name)
    return SR.collect(*loop["cloud"], loop["indices"], loop["best_model"], loop["threshold"])


def index_check_stride(n):
    """A list of INDEX_CHECK_SWEEP + 1 entries into a cloud of n points whose only bad entry is the last one."""
    idx = (np.arange(INDEX_CHECK_SWEEP + 1, dtype=np.uint64) * 7919 % n).astype(np.uint32)
    idx[-1] = n
    return idx


# ------------------------------------------------------------------ ground ----
def ground_600k(n=620000):
    """Three cells of 5 000 points (each longer than a sort tile of 4096 pairs), 250 000 one-point cells and 30 000
    two-point cells, the rest random in a box of +-20."""
    x, y, z = SC._ground_random(600001, n, box=20.0)
    rng = np.random.default_rng(600002)
    at = 0
    for c in range(3):
        x[at:at + 5000] = rng.uniform(30.0 + c, 30.49 + c, 5000).astype(F)
        y[at:at + 5000] = rng.uniform(-30.0, -29.51, 5000).astype(F)
        z[at:at + 5000] = rng.uniform(-0.5, 1.5, 5000).astype(F)
        at += 5000
    k = np.arange(250000)
    x[at:at + 250000] = (100.25 + 0.5 * (k % 600)).astype(F)
    y[at:at + 250000] = (100.25 + 0.5 * (k // 600)).astype(F)
    at += 250000
    k = np.arange(60000) // 2
    x[at:at + 60000] = (-400.25 - 0.5 * (k % 300)).astype(F)
    y[at:at + 60000] = (100.25 + 0.5 * (k // 300)).astype(F)
    p = rng.permutation(n)
    return x[p], y[p], z[p]


@functools.lru_cache(maxsize=None)
def ground_cases():
    large = ground_600k()
    return {
        "n620000": (large, {}),
        "n620000_min1": (large, dict(min_points_per_cell=1, max_ground_height=5.0, cell_percentile=0.5)),
    }


@functools.lru_cache(maxsize=None)
def ground_answer(name):
    cloud, kw = ground_cases()[name]
    return SR.segment_ground(*cloud, **kw)


def compact_without_carry(keep):
    """What count-scan-write leaves of the flags `keep` if k_pack_scan dropped its carry between steps of 1024 block
    counts: the entries' positions, written at offsets that restart with every step (a later write wins)."""
    keep = np.asarray(keep, dtype=bool)
    n = keep.size
    blocks = -(-n // 256)
    padded = np.zeros(blocks * 256, dtype=np.int64)
    padded[:n] = keep
    counts = padded.reshape(blocks, 256).sum(axis=1)
    offsets = np.cumsum(counts) - counts
    step_start = (np.arange(blocks) // 1024) * 1024
    offsets = offsets - offsets[step_start]  # the scan without its carry
    rank = (np.cumsum(padded.reshape(blocks, 256), axis=1) - padded.reshape(blocks, 256)).reshape(-1)[:n]
    pos = np.nonzero(keep)[0]
    out = np.zeros(int(keep.sum()), dtype=np.uint32)
    out[offsets[pos // 256] + rank[pos]] = pos
    return out
