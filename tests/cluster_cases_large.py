"""The large cases of the clustering tests, beside tests/cluster_cases.py so that the small table stays fast.  Their
answers come from their CONSTRUCTION, not from the restatement's Python BFS (which takes minutes at these sizes);
tests/test_cluster_restate.py runs the same constructors at a few thousand points against the BFS and the brute force.

The thresholds, with the kernel and the constant each comes from — when a cap moves, the case named here moves with it:
  SCAN_CHUNK     k_pack_scan scans 1024 block counts per step, a block counts 256 positions: past 262 144 positions the
                 carry between steps is used — Compactor::run over the kept flags (both configurations of blobs_688k keep
                 and reject more than that), k_seg_head_count / k_seg_heads / seg_run_of over the ordered keys
  RS_SMALL_MAX   fdm_rsort.hpp: rs_tile(n) is 1024 pairs up to kRsSmallMax = 600 000, 4096 above: the voxel sort of
                 m = 688 000 pairs and, with min_size 1, the ordering sort of as many take the large tile; with min_size
                 10 the ordering sort has 300 000 pairs, the small tile in a histogram sized for m
  INDEX_SWEEP    k_seg_index_check (fdm_segment.hpp): its grid is capped at 2048 blocks of 256; blobs_688k's list is
                 read by the strided loop, cluster_cases.errors()'s "index_last_of_524289" is refused by it
  chain_300k     k_cluster_merge / k_cluster_flatten: ONE component over 1172 blocks of 256 (the small table's largest
                 is 4097 points, 17 blocks): depth and contention of the union-find across blocks
(The wide keys — more than 32 bits in k_cluster_keys / k_cluster_ranges — are small clouds: tests/cluster_cases.py's
wide_corners and wide_33_bits.)"""
import functools

import numpy as np

import cluster_restate as CR

F = np.float32
SCAN_CHUNK = 1024 * 256
RS_SMALL_MAX = 600000
INDEX_SWEEP = 2048 * 256
TOL = 0.5


def blob_list(n_big, n_small, n_single, seed, unlisted=1000):
    """An index list with duplicates over a smaller cloud, whose partition is known: tight blobs on the lattice of 2^-10
    (every point within +-102/1024 of its blob's centre per axis: a diameter below 0.346 < TOL, every pair of a blob
    neighbours) on a grid of pitch 2.0 (blobs at least 1.6 apart), `n_big` of 10 .. 14 list positions, `n_small` of
    2 .. 9, `n_single` of one; a third of a blob's positions repeat a point of it.  Cloud and list are shuffled apart;
    `unlisted` points of the cloud are in no list entry.  ((x, y, z), indices, the blob of every list position)."""
    rng = np.random.default_rng(seed)
    g = n_big + n_small + n_single
    size = np.concatenate([10 + np.arange(n_big) % 5, 2 + np.arange(n_small) % 8, np.ones(n_single, dtype=np.int64)])
    side = int(np.ceil(g ** (1.0 / 3.0)))
    cell = rng.permutation(side ** 3)[:g]
    centre = (np.stack([cell % side, (cell // side) % side, cell // (side * side)], axis=1) - side // 2) * 2.0
    dup = size // 3
    uniq = size - dup
    blob_of_point = np.repeat(np.arange(g), uniq)
    rank = np.arange(blob_of_point.size) - np.repeat(np.cumsum(uniq) - uniq, uniq)
    pts = centre[blob_of_point] + rng.integers(-102, 103, (blob_of_point.size, 3)) / 1024.0
    again = np.nonzero(rank < dup[blob_of_point])[0]  # a blob's first size // 3 points are listed twice
    entries = np.concatenate([np.arange(blob_of_point.size), again])
    blob = np.concatenate([blob_of_point, blob_of_point[again]])
    # the cloud: the blobs' points and the unlisted ones, shuffled; the list, shuffled on its own
    extra = (rng.integers(0, side, (unlisted, 3)) - side // 2) * 2.0 + rng.integers(-102, 103, (unlisted, 3)) / 1024.0
    cloud = np.concatenate([pts, extra])
    where = rng.permutation(cloud.shape[0])  # point k of `cloud` goes to place where[k]
    shuffled = np.empty_like(cloud)
    shuffled[where] = cloud
    p = rng.permutation(entries.size)
    xyz = tuple(np.ascontiguousarray(shuffled[:, k].astype(F)) for k in range(3))
    assert np.array_equal(np.stack(xyz, axis=1).astype(np.float64), shuffled)  # the lattice is exact in fp32
    return xyz, where[entries[p]].astype(np.uint32), blob[p]


def canonical_of_partition(component, entries, min_size, max_size):
    """The canonical form (cluster_restate.canonical) of a partition given as a component id per list position:
    (indices, offsets, labels, the number of components)."""
    component = np.asarray(component, dtype=np.int64)
    m = component.size
    _, comp = np.unique(component, return_inverse=True)
    size = np.bincount(comp)
    first = np.full(size.size, m, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(m))
    kept = np.nonzero((size >= min_size) & (size <= max_size))[0]
    kept = kept[np.lexsort((first[kept], -size[kept]))]  # descending size, equal sizes by smallest position
    number = np.zeros(size.size, dtype=np.int64)
    number[kept] = np.arange(kept.size) + 1
    labels = number[comp]
    pos = np.nonzero(labels)[0]
    pos = pos[np.argsort(labels[pos], kind="stable")]  # cluster after cluster, positions ascending inside
    offsets = np.concatenate([[0], np.cumsum(size[kept])])
    return entries[pos].astype(np.uint32), offsets.astype(np.uint32), labels.astype(np.uint32), int(size.size)


def chain_long(m, seed):
    """m points 0.875 TOL apart on a line along x — multiples of 7/16, exact in fp32 — their indices shuffled: one
    component (the next point but one is 1.75 TOL away)."""
    k = np.random.default_rng(seed).permutation(m)
    x = (k * 0.4375).astype(F)
    assert np.array_equal(x.astype(np.float64), k * 0.4375)
    return x, np.zeros(m, dtype=F), np.zeros(m, dtype=F)


BLOBS = dict(n_big=25000, n_small=56000, n_single=80000, seed=688)
BLOBS_SMALL = dict(n_big=250, n_small=500, n_single=800, seed=6, unlisted=50)  # the same constructor, for the BFS
CHAIN = 300001


@functools.lru_cache(maxsize=None)
def blobs_688k():
    return blob_list(**BLOBS)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (cloud, keyword arguments of euclidean_cluster, the component of every list position)."""
    cloud, idx, blob = blobs_688k()
    line = chain_long(CHAIN, 300)
    return {
        "blobs_688k_min1": (cloud, dict(tolerance=TOL, min_size=1, indices=idx), blob),
        "blobs_688k_min10": (cloud, dict(tolerance=TOL, min_size=10, indices=idx), blob),
        "chain_300k": (line, dict(tolerance=TOL, max_size=1000000), np.zeros(CHAIN, dtype=np.int64)),
    }


@functools.lru_cache(maxsize=None)
def answer(name):
    """(indices, offsets, labels, n_components) in canonical form, from the construction."""
    cloud, kw, component = cases()[name]
    idx = kw.get("indices")
    entries = np.arange(cloud[0].size, dtype=np.uint32) if idx is None else idx
    return canonical_of_partition(component, entries, kw.get("min_size", 10), kw.get("max_size", 100000))


def on_the_lattice(cloud, indices=None):
    """Every listed coordinate is a multiple of 2^-10 below 2^13: every difference, square and sum of the squared
    distance is exact in fp32 (tests/cluster_cases.py's admission, by construction)."""
    pts, _ = CR._points(*cloud, indices)
    p = pts.astype(np.float64) * 1024.0
    return bool((p == np.round(p)).all() and (np.abs(pts) < 8192.0).all())
