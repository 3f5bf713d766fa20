"""The case table of the clustering tests (tests/test_cluster_restate.py on the CPU, tests/test_cluster_gpu.py on the
GPU): clouds, configurations, and the restatement's answers (tests/cluster_restate.py) in canonical form, computed once
per process and shared.  The rand-free clouds are those of nanoPCL's tests/test_segmentation.cpp (line numbers: that
file's); its rand() scenes are rebuilt with a seeded generator on the same lattices; every other cloud is seeded too.

ADMISSION (asserted by tests/test_cluster_restate.py): a case other than the dyadic ones is here only if every pair of it
whose float64 squared distance lies within r_sq (1 +- 1e-5) gets the same decision under the three fp32 summation orders
and with fused multiply-add.  The seeded scenes are therefore laid on the lattice of 2^-10: there every difference, every
square and every sum of the squared distance is exact in fp32, whatever the order.

Thresholds this table crosses, with the kernel and the constant each comes from (the long lists are in
tests/cluster_cases_large.py, with theirs):
  32 key bits     k_cluster_keys packs [z][y][x] over the voxels' bounding box (cluster::box, at most 21 bits a field) and
                  k_cluster_ranges bisects the sorted keys: wide_33_bits has 11 + 11 + 11, wide_corners 21 + 21 + 21 = 63
  voxel range     cluster_voxel_of accepts -2^20 + range .. 2^20 - 1 - range: wide_corners has blobs AT both ends (range
                  1), errors() "voxel_at_edge" / "voxel_beyond" the first values refused
  index check     k_seg_index_check's grid is capped at 2048 blocks of 256: errors() "index_last_of_524289"."""
import functools

import numpy as np

import cluster_restate as CR

F = np.float32
DYADIC = ("pair_exact", "pair_ulp", "faces_dyadic")  # every operation exact by construction: `<=` decides


def _xyz(pts):
    p = np.asarray(pts, dtype=F).reshape(-1, 3)
    return tuple(np.ascontiguousarray(p[:, k]) for k in range(3))


def _lattice(pts):  # onto the lattice of 2^-10 (exact in fp32 below 2^13)
    return np.round(np.asarray(pts, dtype=np.float64) * 1024.0) / 1024.0


def chain(n, tol, direction, seed, origin=(0.0, 0.0, 0.0)):
    """n points spaced 0.9 tol along `direction`, their indices shuffled."""
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    pts = np.asarray(origin)[None, :] + (0.9 * tol * np.arange(n))[:, None] * d[None, :]
    return _xyz(pts[np.random.default_rng(seed).permutation(n)])


def interleaved_chains(n, tol, seed):
    """two chains 1.5 tol apart, spaced 0.9 tol, point by point in turn, then shuffled"""
    a = np.stack([0.9 * tol * np.arange(n), np.zeros(n), np.zeros(n)], axis=1)
    b = a + np.asarray([0.0, 1.5 * tol, 0.0])[None, :]
    pts = np.empty((2 * n, 3))
    pts[0::2], pts[1::2] = a, b
    return _xyz(pts[np.random.default_rng(seed).permutation(2 * n)])


def multiple_clusters(seed=50):  # createMultipleClusters (:55-74): 50 + 30 + 20 points on the 0.005f lattice
    rng = np.random.default_rng(seed)
    r = lambda k: rng.integers(0, 100, k).astype(F) * F(0.005)  # noqa: E731
    parts = []
    for (cx, cy), k in (((0.0, 0.0), 50), ((5.0, 0.0), 30), ((0.0, 5.0), 20)):
        parts.append(np.stack([F(cx) + r(k), F(cy) + r(k), F(1.0) + r(k)], axis=1))
    return _xyz(np.concatenate(parts))


def two_groups():  # :166-172
    pts = []
    for i in range(20):
        pts += [(F(i) * F(0.1), 0.0, 0.0), (F(10.0) + F(i) * F(0.1), 0.0, 0.0)]
    return _xyz(pts)


def ground_with_obstacles(seed=78):  # createGroundWithObstacles (:78-105)
    rng = np.random.default_rng(seed)
    r = lambda: F(rng.integers(0, 100))  # noqa: E731
    pts = []
    for gx in range(-10, 11):
        for gy in range(-10, 11):
            for _ in range(3):
                pts.append((F(gx) * F(0.5) + r() * F(0.004), F(gy) * F(0.5) + r() * F(0.004), r() * F(0.001)))
    for c in (2.0, -2.0):
        for _ in range(40):
            pts.append((F(c) + r() * F(0.005), F(c) + r() * F(0.005), F(1.0) + r() * F(0.01)))
    return _xyz(pts)


def line_with_noise():  # :259-267
    return _xyz([(F(i) * F(0.1), 0.0, 0.0) for i in range(50)] + [(100.0, 0.0, 0.0), (200.0, 0.0, 0.0)])


def dense_voxel(seed=5000):
    """5 000 points inside the voxel [0, 0.5)^3 of tolerance 0.5: 3 000 in one corner, 2 000 in the opposite one"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 0.08, (3000, 3))
    b = rng.uniform(0.42, 0.499, (2000, 3))
    pts = _lattice(np.concatenate([a, b]))
    return _xyz(pts[rng.permutation(5000)])


def singletons(n=20000, seed=20000):
    """n points at least 0.8 apart (tolerance 0.5): a 1.0 grid, jittered by up to 0.1, shuffled"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(28), np.arange(28), np.arange(26), indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    pts = _lattice(g - 13.0 + rng.uniform(-0.1, 0.1, (n, 3)))
    return _xyz(pts[rng.permutation(n)])


def blobs(count, per, seed, spread=0.14, pitch=3.0, centre=0.0):
    """`count` clusters of exactly `per` points within +-spread of centres `pitch` apart, all points shuffled"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(count)))
    pts = []
    for c in range(count):
        centre_c = np.asarray([(c % side) * pitch + centre, (c // side) * pitch + centre, 0.5])
        pts.append(centre_c[None, :] + rng.uniform(-spread, spread, (per, 3)))
    pts = _lattice(np.concatenate(pts))
    return _xyz(pts[rng.permutation(pts.shape[0])])


def faces_dyadic():
    """points ON voxel faces of tolerance 0.5, negative and positive: a 3 x 3 x 3 lattice of pitch 0.5 (every
    axis-neighbour is exactly the tolerance away: one component of 27) and a second one 4 away, pitch 0.75 (27 singletons)"""
    g = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    return _xyz(np.concatenate([g * 0.5, g * 0.75 + np.asarray([4.0, -4.0, 0.0])]))


def mixed_scene(n=70000, seed=70000):
    """objects of 20 .. 600 points (sigma 0.05 .. 0.4) and a fifth of uniform noise in 100 x 100 x 4, negative
    coordinates included"""
    rng = np.random.default_rng(seed)
    parts, left = [], n - n // 5
    while left > 0:
        k = min(int(rng.integers(20, 600)), left)
        c = np.asarray([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(0, 3)])
        parts.append(c[None, :] + rng.normal(0.0, rng.uniform(0.05, 0.4), (k, 3)))
        left -= k
    parts.append(np.stack([rng.uniform(-50, 50, n // 5), rng.uniform(-50, 50, n // 5), rng.uniform(-1, 3, n // 5)], axis=1))
    pts = _lattice(np.concatenate(parts))
    return _xyz(pts[rng.permutation(n)])


def wide_corners(seed=63):
    """Blobs of 12 .. 20 points at the accepted corner voxels of tolerance 0.5 — -2^20 + 1 and 2^20 - 2 on every axis,
    coordinates on the lattice of 2^-5, which is exact at that magnitude — and blobs near the origin: the voxels' box is
    2^21 - 2 wide on every axis, the sort key 21 + 21 + 21 = 63 bits (k_cluster_keys, k_cluster_ranges' bisection over
    them, eight radix passes).  One corner blob straddles the corner voxel and its inner neighbour."""
    rng = np.random.default_rng(seed)
    lo, hi = (-2.0 ** 20 + 1) * 0.5, (2.0 ** 20 - 2) * 0.5
    parts = []
    for k, corner in enumerate(((lo, lo, lo), (hi, hi, hi), (lo, hi, lo), (hi, lo, hi), (hi, hi, lo))):
        parts.append(np.asarray(corner)[None, :] + rng.integers(0, 8, (12 + 2 * k, 3)) / 32.0)
    parts.append(np.asarray((hi - 0.25, lo, lo))[None, :] + rng.integers(0, 17, (40, 3)) // np.asarray([1, 2, 2]) / 32.0)
    parts.append(np.asarray((lo, lo, lo))[None, :] + np.asarray([[3.0, 0.0, 0.0], [0.0, 3.0, 0.0]]))  # two singletons
    pts = np.concatenate(parts + [np.stack(blobs(6, 15, seed, centre=-2.0), axis=1).astype(np.float64)])
    assert np.array_equal(pts.astype(F).astype(np.float64), pts)
    return _xyz(pts[rng.permutation(pts.shape[0])])


def wide_33_bits(seed=33):
    """Blobs at the origin and 600 away on every axis (voxel 1200: 11 bits a field, a 33-bit key, five radix passes); the
    blob at (0, 0, 600) and the one at (0, 0, 88) differ in bit 32 of the key and above only."""
    rng = np.random.default_rng(seed)
    parts = []
    for k, c in enumerate(((0, 0, 0), (600, 600, 600), (0, 0, 600), (0, 0, 88), (600, 0, 0), (0, 600, 88), (300, 300, 300))):
        parts.append(np.asarray(c, dtype=np.float64)[None, :] + rng.integers(-100, 101, (11 + 3 * k, 3)) / 1024.0)
    pts = np.concatenate(parts)
    return _xyz(pts[rng.permutation(pts.shape[0])])


def sort_keys(cloud, tolerance=0.5, indices=None):
    """(key_bits, the key of every list position): what fdm_cloud_cluster's first sort orders by — [z][y][x] over the
    voxels' bounding box (cluster::box in fdm_cluster_host.hpp)."""
    pts, _ = CR._points(*cloud, indices)
    vox = CR.voxels(pts, CR.relation_constants(tolerance)[0])
    u = vox - vox.min(axis=0)[None, :]
    bits = [max(int(u[:, k].max()).bit_length(), 1) for k in range(3)]
    keys = (u[:, 2] << (bits[0] + bits[1])) | (u[:, 1] << bits[0]) | u[:, 0]
    return sum(bits), keys


KEY_BITS = {"wide_corners": 63, "wide_33_bits": 33}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (cloud, keyword arguments of euclidean_cluster)."""
    mc, gw, tie, mid = multiple_clusters(), ground_with_obstacles(), blobs(64, 12, 6412), blobs(40, 75, 4075, centre=-40.0)
    n_mid = mid[0].size
    rng = np.random.default_rng(99)
    ascending = np.sort(rng.choice(n_mid, n_mid // 2, replace=False)).astype(np.uint32)
    shuffled = rng.permutation(n_mid).astype(np.uint32)[: (2 * n_mid) // 3]
    dup = ascending.copy()
    dup[101] = dup[100]
    up = np.nextafter(F(0.5), F(1.0))
    table = {
        "m0": (_xyz([]), dict()),                                                         # :504-509
        "m1_min2": (_xyz([(1.0, 2.0, 3.0)]), dict(min_size=2)),                           # :523-531
        "m1_min1": (_xyz([(1.0, 2.0, 3.0)]), dict(min_size=1)),
        "m2_far": (_xyz([(0, 0, 0), (3, 0, 0)]), dict(min_size=1)),
        "pair_exact": (_xyz([(0, 0, 0), (0.5, 0, 0)]), dict(tolerance=0.5, min_size=1)),  # exactly tol apart: one cluster
        "pair_ulp": (_xyz([(0, 0, 0), (up, 0, 0)]), dict(tolerance=0.5, min_size=1)),     # one ulp farther: two
        "faces_dyadic": (faces_dyadic(), dict(tolerance=0.5, min_size=1)),
        "interleaved257": (interleaved_chains(257, 0.5, 7), dict(tolerance=0.5)),
        "spheres": (mc, dict(tolerance=1.0, min_size=10, max_size=100)),                  # :111-124
        "spheres_min25": (mc, dict(tolerance=1.0, min_size=25, max_size=100)),            # :192-198
        "spheres_max40": (mc, dict(tolerance=1.0, min_size=10, max_size=40)),             # :200-206
        "two_groups": (two_groups(), dict(tolerance=0.5, min_size=5)),                    # :166-187
        "ground_subset": (gw, dict(tolerance=0.5, min_size=10,                            # :209-234
                                   indices=np.nonzero(gw[2] > F(0.5))[0].astype(np.uint32))),
        "line_noise": (line_with_noise(), dict(tolerance=0.5, min_size=10)),              # :259-277
        "dense_voxel": (dense_voxel(), dict(tolerance=0.5)),
        "singletons_min1": (singletons(), dict(tolerance=0.5, min_size=1)),
        "singletons_min2": (singletons(), dict(tolerance=0.5, min_size=2)),
        "ties64x12": (tie, dict(tolerance=0.5, min_size=10)),
        "negative_tol03": (blobs(30, 40, 303, spread=0.12, pitch=2.0, centre=-30.0), dict(tolerance=0.3)),
        "negative_tol01": (blobs(30, 40, 101, spread=0.04, pitch=1.0, centre=-7.0), dict(tolerance=0.1)),
        "mixed70k": (mixed_scene(), dict(tolerance=0.5)),
        "subset_ascending": (mid, dict(tolerance=0.5, indices=ascending)),
        "subset_shuffled": (mid, dict(tolerance=0.5, indices=shuffled)),
        "subset_duplicate": (mid, dict(tolerance=0.5, indices=dup)),
        "wide_corners": (wide_corners(), dict(tolerance=0.5, min_size=1)),
        "wide_corners_min10": (wide_corners(), dict(tolerance=0.5)),
        "wide_33_bits": (wide_33_bits(), dict(tolerance=0.5)),
    }
    for n in (63, 64, 65, 255, 256, 257, 4097):
        table[f"line{n}"] = (chain(n, 0.5, (1, 0, 0), n), dict(tolerance=0.5))
        table[f"diagonal{n}"] = (chain(n, 0.5, (1, 1, 1), 2 * n, origin=(-300.0, -300.0, -300.0)), dict(tolerance=0.5))
    return table


def list_length(name):
    cloud, kw = cases()[name]
    return cloud[0].size if kw.get("indices") is None else kw["indices"].size


@functools.lru_cache(maxsize=None)
def _core(name):
    cloud, kw = cases()[name]
    pts, entries = CR._points(*cloud, kw.get("indices"))
    clusters, comps = CR.cluster_core(pts, kw.get("tolerance", 0.5), kw.get("min_size", 10), kw.get("max_size", 100000))
    return clusters, len(comps), entries


def restated(name):
    """The restatement's own result: (indices, offsets, clusters as lists of positions in BFS order)."""
    clusters, _, entries = _core(name)
    return (*CR.csr(clusters, entries), clusters)


def n_components(name):
    """... and how many components its BFS grew, the rejected ones included."""
    return _core(name)[1]


@functools.lru_cache(maxsize=None)
def answer(name):
    """The canonical form of the restatement's result: (indices, offsets, labels per list position)."""
    cloud, kw = cases()[name]
    idx = kw.get("indices")
    entries = np.arange(cloud[0].size, dtype=np.uint32) if idx is None else idx
    return CR.canonical(restated(name)[2], entries, entries.size)


@functools.lru_cache(maxsize=None)
def components(name):
    """The brute-force labelling of the case's list positions: label[p] = its component's smallest position."""
    cloud, kw = cases()[name]
    return CR.components_brute(*cloud, kw.get("tolerance", 0.5), kw.get("indices"))


INDEX_CHECK_SWEEP = 2048 * 256


def index_check_stride(n):
    """A list of INDEX_CHECK_SWEEP + 1 entries into a cloud of n points whose only bad entry is the last one."""
    idx = (np.arange(INDEX_CHECK_SWEEP + 1, dtype=np.uint64) * 7919 % n).astype(np.uint32)
    idx[-1] = n
    return idx


@functools.lru_cache(maxsize=None)
def errors():
    """name -> (cloud, keyword arguments, a word of the message): what fdm_cloud_cluster refuses."""
    base = blobs(4, 30, 430)

    def spoiled(axis, at, value):
        c = [v.copy() for v in base]
        c[axis][at] = value
        return tuple(c)

    return {
        "nan": (spoiled(0, 17, np.nan), dict(), "finite"),
        "infinity": (spoiled(2, 99, np.inf), dict(), "finite"),
        "minus_infinity": (spoiled(1, 0, -np.inf), dict(), "finite"),
        "voxel_beyond": (spoiled(0, 5, 524288.0), dict(tolerance=0.5), "voxel"),        # floor(x * 2) = 2^20
        "voxel_at_edge": (spoiled(1, 5, -524288.0), dict(tolerance=0.5), "voxel"),      # -2^20: inside pack, not range
        "tol_zero": (base, dict(tolerance=0.0), "tolerance"),
        "tol_negative": (base, dict(tolerance=-0.5), "tolerance"),
        "tol_nan": (base, dict(tolerance=np.nan), "tolerance"),
        "tol_infinite": (base, dict(tolerance=np.inf), "tolerance"),
        "index_beyond": (base, dict(indices=np.asarray([0, 5, base[0].size, 7], dtype=np.uint32)), "index"),
        # k_seg_index_check's grid is capped at 2048 blocks of 256: entry 524 288 is read by its strided loop only
        "index_last_of_524289": (base, dict(indices=index_check_stride(base[0].size)), "index"),
    }
