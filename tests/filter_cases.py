"""The case tables of the filter tests (tests/test_filter_restate.py on the CPU, tests/test_filter_gpu.py on the GPU):
clouds, radii, and the restatement's answers (tests/filter_restate.py), computed once per process and shared.

RADIUS OUTLIER REMOVAL.  Every cloud whose answer is compared exactly lies on the lattice of 2^-10 below 2^13
(cluster_cases_large.on_the_lattice) or is one of tests/cluster_cases.py's admitted clouds: there every difference, square
and sum of the squared distance is exact in fp32, so `<=` decides whatever the summation order.

Thresholds this table crosses, with the kernel and the constant each comes from:
  block edges     k_ror_candidates / k_ror_count: blocks of 256 — line255, line256, line257
  sort's tile     fdm_rsort.hpp: more than one tile of 1024 pairs — line4097; rs_tile(n) is 4096 past kRsSmallMax = 600 000 —
                  large() (610 000 points), whose answer comes from its construction
  32 key bits     k_cluster_keys packs [z][y][x] over the voxels' bounding box, the bisections of k_ror_candidates /
                  k_ror_count compare whole keys: wide_33_bits (11 + 11 + 11)
  early exit      mask mode walks a point's own row first and stops at min_neighbors: dense_voxel (5 000 points in one voxel,
                  two true outliers in neighbouring voxels)
  voxel range     errors() "voxel_beyond": a coordinate at 2^20 * radius
  work bound      filter::kMaxTests (fdm_filter_host.hpp): 560 000 points in one voxel, built on the device by the test

A RADIUS WHOSE RANGE IS 2.  range = int(ceil(radius * (1.0f / radius))) is 2 iff the fp32 product exceeds 1.
range_two_radius() searches EVERY fp32 radius of the binade [1, 2) — 2^23 values; scaling a radius by a power of two
scales the reciprocal exactly, so the binade stands for every normal radius — and finds none: round-to-nearest leaves
fl(1 / r) within a relative 2^-24 / (1 + 2^-24) of 1 / r, and a product below 1 + 2^-24 rounds to 1.  So there is no such
case in this table: the kernel's 25-row walk is reached by no fp32 radius, and cluster::relation refuses what is left (a
reciprocal that overflowed)."""
import functools

import numpy as np

import cluster_cases as CC
import cluster_cases_large as CL
import filter_restate as FR

F = np.float32
STEP = 1.0 / 1024.0


def _pts(cloud):
    return np.stack([np.asarray(v, dtype=F) for v in cloud], axis=1) if cloud[0].size else np.zeros((0, 3), dtype=F)


@functools.lru_cache(maxsize=None)
def range_two_radius():
    """The first fp32 radius of [1, 2) with radius * (1.0f / radius) > 1, or None (see the module's text)."""
    r = (np.arange(1 << 23, dtype=np.uint32) + np.uint32(0x3F800000)).view(F)
    hit = np.nonzero(r * (F(1.0) / r) > F(1.0))[0]
    return None if hit.size == 0 else F(r[hit[0]])


def blob40(seed=40):
    """40 points within +-60/1024 of the origin: every pair within 0.21 < 0.5, every count 39"""
    rng = np.random.default_rng(seed)
    return CC._xyz(rng.integers(-60, 61, (40, 3)) * STEP)


def exact_radius():
    """Neighbours at exactly the radius 0.5 along every axis, negative side included, and at 0.5 + 2^-10: the centre has
    6 neighbours (`<=`), each of them only the centre; the five points whose nearest point is one lattice step farther
    than the radius have none."""
    near = [(0.5, 0, 0), (-0.5, 0, 0), (0, 0.5, 0), (0, -0.5, 0), (0, 0, 0.5), (0, 0, -0.5)]
    far = [(8.0, 8.0, 8.0), (8.5 + STEP, 8.0, 8.0), (8.0, 8.0 - 0.5 - STEP, 8.0), (-8.0, -8.0, -8.0), (-8.0, -8.0, -8.5 - STEP)]
    return CC._xyz([(0, 0, 0)] + near + far)


def signed_zeros():
    """-0.0 and +0.0 are one voxel and one place: four points at the origin (counts 3) and a blob of the negative octant"""
    rng = np.random.default_rng(7)
    zeros = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0)]
    blob = -rng.integers(1, 300, (30, 3)) * STEP
    return CC._xyz(np.concatenate([np.asarray(zeros), blob]))


def dense_voxel(seed=5002):
    """5 000 points inside [0, 80/1024]^3 of the voxel [0, 0.5)^3 and two true outliers in neighbouring voxels: one in the
    same (y, z) row — voxel (1, 0, 0), inside the own-row interval — and one in the row above, voxel (0, 1, 0)."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.integers(0, 81, (5000, 3)) * STEP, np.asarray([[0.9375, 0.0, 0.0], [0.0, 0.9375, 0.0]])])
    return CC._xyz(pts[rng.permutation(5002)])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (cloud, radius, min_neighbors)."""
    n40 = 40
    table = {
        "n0": (CC._xyz([]), 0.5, 1),
        "n1": (CC._xyz([(1.0, 2.0, 3.0)]), 0.5, 1),
        "n1_min0": (CC._xyz([(1.0, 2.0, 3.0)]), 0.5, 0),
        "n2_duplicate": (CC._xyz([(1.0, 2.0, 3.0), (1.0, 2.0, 3.0)]), 0.5, 1),  # j != i by index: each counts the other
        "n2_far": (CC._xyz([(0, 0, 0), (3, 0, 0)]), 0.5, 1),
        "blob40_min0": (blob40(), 0.5, 0),
        "blob40_min1": (blob40(), 0.5, 1),
        "blob40_min_n_1": (blob40(), 0.5, n40 - 1),
        "blob40_min_n": (blob40(), 0.5, n40),
        "exact_radius": (exact_radius(), 0.5, 1),
        "faces_dyadic": (CC.faces_dyadic(), 0.5, 4),
        "signed_zeros": (signed_zeros(), 0.5, 3),
        "negative_r03": (CC.blobs(30, 40, 303, spread=0.12, pitch=2.0, centre=-30.0), 0.3, 38),
        "negative_r01": (CC.blobs(30, 40, 101, spread=0.04, pitch=1.0, centre=-7.0), 0.1, 38),
        "spheres_r1": (CC.multiple_clusters(), 1.0, 25),
        "wide_33_bits": (CC.wide_33_bits(), 0.5, 15),
        "dense_voxel": (dense_voxel(), 0.5, 5),
        "mixed_r05": (CC.mixed_scene(6000, 6000), 0.5, 5),
    }
    for n in (255, 256, 257, 4097):
        table[f"line{n}"] = (CC.chain(n, 0.5, (1, 0, 0), n), 0.5, 2)  # the two ends have one neighbour
    return table


KEY_BITS = {"wide_33_bits": 33}
LATTICE_FREE = ("spheres_r1",) + tuple(f"line{n}" for n in (255, 256, 257, 4097))  # admitted by tests/cluster_cases.py


@functools.lru_cache(maxsize=None)
def counts(name):
    """The restatement's neighbour counts at the reference's table and chain level."""
    cloud, radius, _ = cases()[name]
    return FR.radius_counts_reference(_pts(cloud), radius)


@functools.lru_cache(maxsize=None)
def brute(name):
    cloud, radius, _ = cases()[name]
    return FR.radius_counts_brute(_pts(cloud), radius)


# ---- the large case: its answer comes from its construction ----
RADIUS = 0.5
LARGE = dict(n_blobs=80000, n_pairs=20000, n_single=50000, seed=610)
LARGE_SMALL = dict(n_blobs=600, n_pairs=150, n_single=400, seed=61)  # the same constructor, for the restatements


def blob_cloud(n_blobs, n_pairs, n_single, seed):
    """Tight blobs of 2 .. 11 points (every point within +-102/1024 of its blob's centre per axis: a diameter below
    0.346 < RADIUS), pairs of points EXACTLY RADIUS apart along x, and singletons, on a grid of pitch 2.0 (anything of
    two different cells is at least 1.2 apart), on the lattice of 2^-10, shuffled.  A blob point counts its blob's size
    - 1 (a repeated coordinate is another point), a pair's point 1, a singleton 0.  ((x, y, z), the count of every point)."""
    rng = np.random.default_rng(seed)
    g = n_blobs + n_pairs + n_single
    side = int(np.ceil(g ** (1.0 / 3.0)))
    cell = rng.permutation(side ** 3)[:g]
    centre = (np.stack([cell % side, (cell // side) % side, cell // (side * side)], axis=1) - side // 2) * 2.0
    size = 2 + np.arange(n_blobs) % 10
    blob_of = np.repeat(np.arange(n_blobs), size)
    blobs = centre[blob_of] + rng.integers(-102, 103, (blob_of.size, 3)) * STEP
    first = centre[n_blobs:n_blobs + n_pairs]
    pts = np.concatenate([blobs, first, first + np.asarray([RADIUS, 0.0, 0.0]), centre[n_blobs + n_pairs:]])
    want = np.concatenate([size[blob_of] - 1, np.ones(2 * n_pairs, dtype=np.int64), np.zeros(n_single, dtype=np.int64)])
    p = rng.permutation(pts.shape[0])
    cloud = tuple(np.ascontiguousarray(pts[p, k].astype(F)) for k in range(3))
    assert np.array_equal(np.stack(cloud, axis=1).astype(np.float64), pts[p])  # the lattice is exact in fp32
    return cloud, want[p].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def large():
    return blob_cloud(**LARGE)


# ---- what fdm_cloud_radius_outlier_removal refuses ----
@functools.lru_cache(maxsize=None)
def errors():
    """name -> (cloud, radius, a word of the message)."""
    base = CC.blobs(4, 30, 430)

    def spoiled(axis, at, value):
        c = [v.copy() for v in base]
        c[axis][at] = value
        return tuple(c)

    return {
        "nan": (spoiled(0, 17, np.nan), 0.5, "finite"),
        "infinity": (spoiled(2, 99, np.inf), 0.5, "finite"),
        "voxel_beyond": (spoiled(0, 5, 2.0 ** 20 * 0.5), 0.5, "voxel"),  # a coordinate at 2^20 * radius
    }


# ---- the crop cloud and its cases ----
PI = float(F(np.pi))


@functools.lru_cache(maxsize=None)
def crop_cloud(n=1000, seed=1000):
    """n points of a normal cloud (sigma 3), seeded with NaN, +-inf, +-0.0, coordinates EQUAL TO the bounds of
    crop_cases(), points exactly on both spheres of the range crops, on the boundary rays of the angle crops and at the
    origin."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0.0, 3.0, (n, 3)).astype(F)
    nan, inf = np.nan, np.inf
    c45, s45 = np.cos(np.pi / 4), np.sin(np.pi / 4)
    special = [
        (nan, 0.5, 0.5), (0.5, nan, 0.5), (0.5, 0.5, nan), (nan, nan, nan), (nan, 5.0, 0.5), (nan, -5.0, 0.5),
        (inf, 0.0, 0.0), (-inf, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf), (inf, -inf, inf), (inf, nan, 0.0),
        (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0), (-0.0, 0.0, 1.0),
        # the box's and the axes' bounds themselves: lo = (-1, -2, 0), hi = (2, 1, 1.5)
        (-1.0, -2.0, 0.0), (2.0, 1.0, 1.5), (-1.0, 1.0, 1.5), (2.0, -2.0, 0.0), (0.5, 0.5, 1.5), (0.5, 0.5, 0.0),
        (np.nextafter(F(2.0), F(3.0)), 0.0, 0.5), (np.nextafter(F(-1.0), F(-2.0)), 0.0, 0.5), (0.0, 0.0, np.nextafter(F(1.5), F(2.0))),
        # exactly on the spheres of radius 1 and 5, and one ulp off
        (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (3.0, 4.0, 0.0), (0.0, -3.0, 4.0), (5.0, 0.0, 0.0),
        (np.nextafter(F(5.0), F(6.0)), 0.0, 0.0), (np.nextafter(F(1.0), F(0.0)), 0.0, 0.0),
        # on the boundary rays of (-pi/4, pi/4), of (3, -3) and of (0, pi); behind the sensor; on the axes
        (1.0, 1.0, 0.0), (1.0, -1.0, 0.0), (2.0, 2.0, 3.0), (c45, s45, 0.0), (c45, -s45, 0.0), (-1.0, 1.0, 0.0), (-1.0, -1.0, 0.0),
        (np.cos(3.0), np.sin(3.0), 0.0), (np.cos(-3.0), np.sin(-3.0), 0.0), (-4.0, 0.0, 0.0), (-4.0, 1e-5, 0.0), (-4.0, -1e-5, 0.0),
        (4.0, 0.0, 0.0), (0.0, 4.0, 0.0), (0.0, -4.0, 0.0), (1.0, 1e-5, 0.0), (1.0, -1e-5, 0.0), (1e-6, 1e-6, 0.0), (1e6, 1.0, 0.0),
        (np.cos(2.0), np.sin(2.0), 0.0), (np.cos(-2.0), np.sin(-2.0), 0.0),
    ]
    at = rng.permutation(n)[:len(special)]
    p[at] = np.asarray(special, dtype=F)
    return tuple(np.ascontiguousarray(p[:, k]) for k in range(3))


@functools.lru_cache(maxsize=None)
def crop_cases():
    """name -> (function of fastdem_amd, its arguments after x, y, z; the restatement's keep mask for "inside" and for
    "outside" — remove_invalid has one).  min > max is covered for every kind that has bounds."""
    x, y, z = crop_cloud()
    lo, hi = (-1.0, -2.0, 0.0), (2.0, 1.0, 1.5)
    table = {}

    def both(name, fn, args, restate):
        table[name] = (fn, args, {m: restate(m) for m in ("inside", "outside")})

    both("box", "crop_box", (lo, hi), lambda m: FR.crop_box(x, y, z, lo, hi, m))
    both("box_min_above_max", "crop_box", ((1.0, -2.0, 0.0), (-1.0, 1.0, 1.5)),
         lambda m: FR.crop_box(x, y, z, (1.0, -2.0, 0.0), (-1.0, 1.0, 1.5), m))
    both("range", "crop_range", (1.0, 5.0), lambda m: FR.crop_range(x, y, z, 1.0, 5.0, m))
    both("range_min_above_max", "crop_range", (5.0, 1.0), lambda m: FR.crop_range(x, y, z, 5.0, 1.0, m))
    both("range_from_zero", "crop_range", (0.0, 1.0), lambda m: FR.crop_range(x, y, z, 0.0, 1.0, m))
    for axis, v, fn in ((0, x, "crop_x"), (1, y, "crop_y"), (2, z, "crop_z")):
        both(fn, fn, (lo[axis], hi[axis]), lambda m, v=v, a=axis: FR.crop_axis(v, lo[a], hi[a], m))
        both(fn + "_min_above_max", fn, (hi[axis], lo[axis]), lambda m, v=v, a=axis: FR.crop_axis(v, hi[a], lo[a], m))
        both(fn + "_one_value", fn, (hi[axis], hi[axis]), lambda m, v=v, a=axis: FR.crop_axis(v, hi[a], hi[a], m))
    for name, a, b in (("angle_quarter", -PI / 4, PI / 4), ("angle_wrapped", 3.0, -3.0), ("angle_wide", -2.0, 2.0),
                       ("angle_exactly_pi", 0.0, PI), ("angle_one_ray", 1.0, 1.0), ("angle_wrapped_wide", 1.0, -1.0)):
        both(name, "crop_angle", (a, b), lambda m, a=a, b=b: FR.crop_angle(x, y, z, a, b, m))
    table["finite"] = ("remove_invalid", (), {"inside": FR.remove_invalid(x, y, z)})
    return table


GRID_EDGE = 1024 * 256 + 1  # k_filter_keep's grid is capped at kFilterMaxBlocks = 1024 blocks of 256: the strided loop's first point
