"""The case table of the segmentation tests (tests/test_seg_restate.py on the CPU, tests/test_segment_gpu.py on the
GPU): clouds, configurations, and the restatement's answers (tests/seg_restate.py), computed once per process and shared.
The rand-free clouds are those of nanoPCL's tests/test_segmentation.cpp (line numbers: that file's); every other cloud is
seeded, so neither test needs a reference file.

Thresholds this table crosses, with the kernel and the constant each comes from (the long lists are in
tests/seg_cases_large.py, with theirs):
  32 key bits     k_seg_pack_keys packs [gy][gx] over the cells' bounding box and fdm_cloud_segment_ground's second sort
                  takes bits_x + bits_y bits of it (seg_bits, eight per radix pass): wide_bits33 has 17 + 16, wide_bits64
                  and wide_extremes 32 + 32 — bits_x = 32, where the shift is a whole word
  int32 floors    seg_cell_of accepts floor(v / r) in [-2^31, 2^31): wide_extremes holds both ends, ground_errors()
                  "floor_exactly_2_31" the first value refused"""
import functools

import numpy as np

import seg_restate as SR

F = np.float32
BATCH = 128  # the engine's default hypotheses per launch (fdm_segment_stats.batch)


def _xyz(pts):
    p = np.asarray(pts, dtype=F).reshape(-1, 3)
    return tuple(np.ascontiguousarray(p[:, k]) for k in range(3))


# ------------------------------------------------------------------ planes ----
def grid_cloud(z_values, nx=10, ny=10):  # :292-299, :327-341
    return _xyz([(float(x), float(y), zv) for zv in z_values for x in range(nx) for y in range(ny)])


def line_cloud():  # :354-357
    return _xyz([(float(i), 0.0, 0.0) for i in range(10)])


def scene(seed, n, fraction, planes=((0.05, -0.03, 0.4),), noise=0.02, box=10.0):
    """n points in a box of +-`box`: of plane q (z = a x + b y + c) a share fraction[q] within +-noise of it, the rest
    uniform in the box; shuffled."""
    rng = np.random.default_rng(seed)
    fraction = (fraction,) if np.isscalar(fraction) else fraction
    parts = []
    for (a, b, c), f in zip(planes, fraction):
        k = int(round(n * f))
        px, py = rng.uniform(-box, box, k), rng.uniform(-box, box, k)
        parts.append(np.stack([px, py, a * px + b * py + c + rng.uniform(-noise, noise, k)], axis=1))
    k = n - sum(p.shape[0] for p in parts)
    parts.append(rng.uniform(-box, box, (k, 3)))
    pts = np.concatenate(parts)
    return _xyz(pts[rng.permutation(n)])


def _with_bad_points(cloud):
    x, y, z = (v.copy() for v in cloud)
    x[3], y[10], z[17], x[40], z[41] = np.nan, np.inf, -np.inf, np.nan, np.nan
    return x, y, z


@functools.lru_cache(maxsize=None)
def plane_cases():
    """name -> (cloud, keyword arguments of segment_plane)."""
    s45, s30, s20, s12 = (scene(seed, 500, f) for seed, f in ((145, 0.45), (130, 0.30), (120, 0.20), (112, 0.12)))
    third = np.arange(0, 500, 3, dtype=np.uint32)
    third[7] = third[6]  # a duplicate
    cases = {
        "grid_z1": (grid_cloud([1.0]), dict(distance_threshold=0.1)),                      # :292-307: runs to the cap
        "two_planes": (grid_cloud([0.0, 5.0]), dict(distance_threshold=0.1, max_iterations=500)),  # :326-345
        "line10": (line_cloud(), dict(distance_threshold=0.1, max_iterations=100)),         # :352-364
        "one_point": (_xyz([(1.0, 2.0, 3.0)]), dict(distance_threshold=0.1)),               # :523-535
        "two_points": (_xyz([(0, 0, 0), (1, 0, 0)]), dict(distance_threshold=0.1)),         # :542-548
        "zero_points": (_xyz([]), dict(distance_threshold=0.1)),                            # :511-515
        "scene45": (s45, dict(distance_threshold=0.05)),
        "scene30": (s30, dict(distance_threshold=0.05)),
        "scene20": (s20, dict(distance_threshold=0.05)),
        "scene12": (s12, dict(distance_threshold=0.05)),
        "scene30_cap100": (s30, dict(distance_threshold=0.05, max_iterations=100)),
        "scene45_third": (s45, dict(distance_threshold=0.05, indices=third)),
        "scene45_nan_inf": (_with_bad_points(s45), dict(distance_threshold=0.05)),
        "scene45_min_inliers": (s45, dict(distance_threshold=0.05, min_inliers=400)),
        "scene45_unrefined": (s45, dict(distance_threshold=0.05, refine_model=False)),
        "scene20_unrefined": (s20, dict(distance_threshold=0.05, refine_model=False)),
        "scene70k": (scene(170, 70000, 0.5), dict(distance_threshold=0.05)),
    }
    return cases


# what the table promises about the loop (asserted on the CPU): the batches a case's loop passes span
WITHIN_ONE_BATCH = ("scene45",)
ACROSS_BATCH_EDGES = ("scene20", "scene20_unrefined")  # >= 2 batch edges each (scene30 crosses one)
AT_THE_CAP = ("scene12", "grid_z1", "scene30_cap100")
INDEX_ERROR = (scene(145, 500, 0.45), dict(distance_threshold=0.05, indices=np.array([0, 5, 500, 7], dtype=np.uint32)))


@functools.lru_cache(maxsize=None)
def plane_answer(name, order="forward", solver="eigh"):
    cloud, kw = plane_cases()[name]
    return SR.segment_plane(*cloud, order=order, solver=solver, **kw)


def three_planes():
    # (the third plane holds 2 % of the points: about 8 % of what the first two leave, below min_fitness 0.1)
    return scene(333, 3000, (0.45, 0.30, 0.02), planes=((0.05, -0.03, 0.4), (-0.2, 0.1, 3.0), (0.3, 0.3, -4.0)))


@functools.lru_cache(maxsize=None)
def multi_cases():
    """name -> (cloud, keyword arguments of segment_multiple_planes)."""
    return {
        "two_planes": (grid_cloud([0.0, 5.0]), dict(distance_threshold=0.1, max_iterations=500, max_planes=3,
                                                    min_fitness=0.1)),                      # :326-349
        "three_planes": (three_planes(), dict(distance_threshold=0.05, max_planes=5, min_fitness=0.1)),
    }


@functools.lru_cache(maxsize=None)
def multi_answer(name, order="forward", solver="eigh"):
    cloud, kw = multi_cases()[name]
    return SR.segment_multiple_planes(*cloud, order=order, solver=solver, **kw)


# ------------------------------------------------------------------ ground ----
def _ground_random(seed, n, box=6.0):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-box, box, n).astype(F), rng.uniform(-box, box, n).astype(F)
    z = (rng.uniform(0.0, 0.2, n) + (rng.uniform(0, 1, n) < 0.2) * rng.uniform(0.3, 2.0, n)).astype(F)
    return x, y, z


def ground_edges(seed=255, n=255):
    """Negative coordinates and points exactly on cell edges of the 0.5 grid."""
    x, y, z = _ground_random(seed, n, box=3.0)
    k = np.arange(0, n, 4)
    x[k] = (np.round(x[k] / 0.5) * 0.5).astype(F)
    y[k[::2]] = (np.round(y[k[::2]] / 0.5) * 0.5).astype(F)
    return x, y, z


def ground_thirds(n=257):
    """Coordinates k * 0.3f on a 0.3f grid: x / r and x * (1 / r) floor differently at some of them."""
    r = F(0.3)
    k = np.arange(n, dtype=np.int64) - 100
    rng = np.random.default_rng(257)
    x = (k.astype(F) * r).astype(F)
    y = (rng.integers(-3, 4, n).astype(F) * r).astype(F)
    z = rng.uniform(0.0, 1.0, n).astype(F)
    return x, y, z


def divide_and_multiply_differ(v, r):
    r = F(r)
    inv = F(F(1.0) / r)
    return np.floor((v / r).astype(F)) != np.floor((v * inv).astype(F))


def ground_exact_cut(n=4097):
    """One cell whose points sit exactly AT robust + thickness (ground: the comparison is strict) and one ulp above it
    (obstacles); a cell whose robust minimum is above max_ground_height; -0.0 beside +0.0; the rest random."""
    x, y, z = _ground_random(4097, n)
    # cell (20, 20) of the 0.5 grid: fourteen points, the ten lowest z = 0.10 .. 0.19, the other four at the cut and just
    # above it: idx = size_t(0.2f * 13) = 2, robust = 0.12f
    base = (F(0.10) + np.arange(10, dtype=F) * F(0.01)).astype(F)
    robust = np.sort(base)[int(F(0.2) * F(13))]
    cut = F(robust + F(0.3))
    x[:14], y[:14] = F(10.2), F(10.3)
    z[:10] = base[::-1]
    z[10], z[11] = cut, cut
    z[12], z[13] = np.nextafter(cut, F(np.inf)), np.nextafter(cut, F(np.inf))
    # cell (-30, -30): its robust minimum 0.8 is above max_ground_height 0.5 although one point is low
    x[14:24], y[14:24] = F(-14.9), F(-14.8)
    z[14:24] = F(0.8)
    z[14] = F(0.0)
    # cell (30, -30): zeros of both signs
    x[24:30], y[24:30] = F(15.1), F(-14.7)
    z[24:30] = np.array([0.0, -0.0, 0.0, -0.0, -0.0, 0.0], dtype=F)
    return x, y, z


def ground_large(n=70000):
    """A cell of 5 000 points (longer than a sort tile), 20 000 one-point cells, the rest random."""
    x, y, z = _ground_random(70000, n, box=20.0)
    rng = np.random.default_rng(70001)
    x[:5000] = rng.uniform(30.0, 30.49, 5000).astype(F)
    y[:5000] = rng.uniform(30.0, 30.49, 5000).astype(F)
    z[:5000] = rng.uniform(-0.5, 1.5, 5000).astype(F)
    k = np.arange(20000)
    x[5000:25000] = (100.25 + 0.5 * (k % 200)).astype(F)
    y[5000:25000] = (100.25 + 0.5 * (k // 200)).astype(F)
    p = rng.permutation(n)
    return x[p], y[p], z[p]


def ground_wide(kind, n=300):
    """A cloud of n points whose cell box (resolution 0.5) is too wide for a 32-bit cell key — k_seg_pack_keys packs
    [gy][gx] over the box and the second sort takes bits_x + bits_y bits of it:
      "bits33"    2^17 x 2^16 cells: 17 + 16 bits, five radix passes
      "bits64"    groups near x, y = +-1.0e9 (cells near +-2.0e9): 32 + 32 bits, eight passes, a shift by a whole word
      "extremes"  the same widths from the accepted extremes themselves: a floor of exactly -2^31 and the largest float
                  below 2^31
    Twenty groups of six points with exactly equal x, y and different z, so that runs and the percentile pick happen at
    those magnitudes; the groups come in pairs (P, Q) in cells that differ in a key bit above 31 only: P's z is
    0 .. 0.1, Q's 0.35 .. 0.45 — ground in a cell of its own, obstacles if Q were taken for a part of P's cell.  The other
    points share a few hundred cells inside the box, one to a few each."""
    rng = np.random.default_rng({"bits33": 33, "bits64": 64, "extremes": 31}[kind])
    if kind == "bits33":   # coordinates k / 2 + 0.25: exact
        px = np.concatenate([[0, 2 ** 17 - 1], rng.integers(0, 2 ** 17, 8)]) * 0.5 + 0.25
        py = np.concatenate([[0, 2 ** 15 - 1], rng.integers(0, 2 ** 15, 8)]) * 0.5 + 0.25
        qx, qy = px, py + 2.0 ** 14  # 2^15 cells on: bit 15 of gy, bit 32 of the key
        fx = rng.integers(0, 2 ** 17, 20)[rng.integers(0, 20, n)] * 0.5 + 0.25
        fy = rng.integers(0, 2 ** 16, 20)[rng.integers(0, 20, n)] * 0.5 + 0.25
    else:                  # floats near 1e9 are 64 apart, those below 2^30 too
        lo, hi = (-1.0e9, 1.0e9) if kind == "bits64" else (-2.0 ** 30, 2.0 ** 30 - 64.0)
        step = 64.0 * rng.integers(0, 1000, 10)
        px = np.where(np.arange(10) % 2 == 0, lo + step, hi - step)
        px[:2] = lo, hi
        py = np.full(10, lo) + 64.0 * np.arange(10)
        qx, qy = px, np.full(10, hi) - 64.0 * np.arange(10)  # the same gx, the far end of gy
        fx = np.where(rng.integers(0, 2, n) == 0, lo, hi) + 64.0 * rng.integers(-8, 9, n) * (1 if kind == "bits64" else 0)
        fy = rng.integers(-2 ** 23, 2 ** 23, 30)[rng.integers(0, 30, n)] * 64.0
    gx, gy = np.repeat(np.concatenate([px, qx]), 6), np.repeat(np.concatenate([py, qy]), 6)
    gz = np.concatenate([rng.uniform(0.0, 0.1, 60), rng.uniform(0.35, 0.45, 60)])
    k = n - 120
    x, y = np.concatenate([gx, fx[:k]]), np.concatenate([gy, fy[:k]])
    z = np.concatenate([gz, rng.uniform(0.0, 1.0, k)])
    p = rng.permutation(n)
    cloud = x[p].astype(F), y[p].astype(F), z[p].astype(F)
    assert np.array_equal(cloud[0].astype(np.float64), x[p]) and np.array_equal(cloud[1].astype(np.float64), y[p])
    return cloud


def ground_key_bits(cloud, resolution=0.5):
    """(bits_x, bits_y, the packed key of every point): what fdm_cloud_segment_ground sorts by."""
    gx, gy = (SR.cell_coordinates(v, resolution).astype(np.int64) for v in cloud[:2])
    ex, ey = int(gx.max() - gx.min()), int(gy.max() - gy.min())
    bits_x, bits_y = max(ex.bit_length(), 1), max(ey.bit_length(), 1)
    keys = [(int(b - gy.min()) << bits_x) | int(a - gx.min()) for a, b in zip(gx, gy)]
    return bits_x, bits_y, keys


def ground_with_32_bit_keys(cloud, **kw):
    """The restatement's answer if only the low 32 bits of the packed cell key were sorted and compared (four radix
    passes instead of bits / 8): points whose keys agree there share a cell."""
    _, _, keys = ground_key_bits(cloud, kw.get("grid_resolution", 0.5))
    low = np.array([k & 0xFFFFFFFF for k in keys], dtype=np.int64)
    res = kw.get("grid_resolution", 0.5)
    sx, sy = ((low % 65536) * res + res / 2).astype(F), ((low // 65536) * res + res / 2).astype(F)  # one cell per low key
    return SR.segment_ground(sx, sy, cloud[2], **kw)


@functools.lru_cache(maxsize=None)
def ground_cases():
    """name -> (cloud, keyword arguments of segment_ground)."""
    one = _xyz([(1.0, 2.0, 3.0)])
    two = (np.array([0.1, 0.2], dtype=F), np.array([0.1, 0.2], dtype=F), np.array([-0.0, 0.0], dtype=F))
    edges, thirds, exact, large = ground_edges(), ground_thirds(), ground_exact_cut(), ground_large()
    cases = {
        "n1": (one, {}),
        "n1_min1": (one, dict(min_points_per_cell=1)),
        "n1_min0": (one, dict(min_points_per_cell=0)),
        "n1_min1_high": (one, dict(min_points_per_cell=1, max_ground_height=5.0)),
        "n2_zeros": (two, {}),
        "n255_edges": (edges, {}),
        "n255_p0": (edges, dict(cell_percentile=0.0)),
        "n255_p1": (edges, dict(cell_percentile=1.0)),
        "n255_p1_5": (edges, dict(cell_percentile=1.5)),
        "n255_min1": (edges, dict(min_points_per_cell=1)),
        "n255_min0": (edges, dict(min_points_per_cell=0, grid_resolution=2.0)),
        "n257_thirds": (thirds, dict(grid_resolution=0.3, max_ground_height=2.0)),
        "n4097_exact_cut": (exact, {}),
        "n4097_coarse": (exact, dict(grid_resolution=2.0, ground_thickness=0.1)),
        "n70000": (large, {}),
        "n70000_p1": (large, dict(cell_percentile=1.0, max_ground_height=5.0, min_points_per_cell=1)),
    }
    for kind in GROUND_WIDE:
        cases["wide_" + kind] = (ground_wide(kind), {})
        cases["wide_" + kind + "_min1"] = (ground_wide(kind), dict(min_points_per_cell=1, cell_percentile=0.5))
    return cases


GROUND_WIDE = {"bits33": (17, 16), "bits64": (32, 32), "extremes": (32, 32)}  # kind -> (bits_x, bits_y)


@functools.lru_cache(maxsize=None)
def ground_answer(name):
    cloud, kw = ground_cases()[name]
    return SR.segment_ground(*cloud, **kw)


def ground_errors():
    """name -> (cloud, keyword arguments): the inputs at which the reference is undefined."""
    x, y, z = ground_edges()
    bad_nan, bad_inf, far, first = x.copy(), z.copy(), y.copy(), x.copy()
    bad_nan[100] = np.nan
    bad_inf[7] = np.inf
    far[200] = F(3.0e9)  # floor(3e9 / 0.5) is outside int32
    first[31] = F(2.0 ** 30)  # floor(2^30 / 0.5) = 2^31 exactly: the first floor that is refused
    return {
        "nan_coordinate": ((bad_nan, y, z), {}),
        "inf_z": ((x, y, bad_inf), {}),
        "floor_outside_int32": ((x, far, z), {}),
        "floor_exactly_2_31": ((first, y, z), {}),
        "resolution_zero": ((x, y, z), dict(grid_resolution=0.0)),
        "resolution_negative": ((x, y, z), dict(grid_resolution=-0.5)),
        "resolution_inf": ((x, y, z), dict(grid_resolution=float("inf"))),
        "resolution_nan": ((x, y, z), dict(grid_resolution=float("nan"))),
        "percentile_nan": ((x, y, z), dict(cell_percentile=float("nan"))),
        "percentile_negative": ((x, y, z), dict(cell_percentile=-0.1)),
    }
