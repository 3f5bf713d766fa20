"""Clouds for the limits of floating-point removal and buildDEM (tests/test_dem_restate.py proves on the CPU which path of
the two sorts, of k_hf_peak and of the compaction each one reaches; tests/test_dem_edges_gpu.py runs them on the device),
and the restatement's answers to them, computed once per process.  Test data, not product.

Filter cases (Engine.remove_floating_points against DR.restate_floating_grouped):
  bins_2, bins_3, bins_4   one cloud on 260 x 260 cells; bin sizes that give the bin sort 2, 3 and 4 passes
  cells_1, cells_256, cells_4   maps of 255, 256 and 4 097 x 4 096 cells: the cell sort's 1 and 4 passes, the skip key's bit
  long_run                 a cell of 5 000 points over 410 bins with a tied peak, a cell of 1 025 points in one bin
  tile_large               600 001 pairs (tiles of 4 096), 20 000 of them with a z
  moved                    a map whose start index is not (0, 0)
Pipeline cases (gpu.build_dem against DR.restate_build_dem): none_survive_*, minus_one_metre, one_cell, one_row, utm,
scan_chunks, refused_late, fallback.
"""
import collections
import functools
import time

import numpy as np

import dem_restate as DR
import test_build_dem_gpu as TB

F32 = np.float32

FilterCase = collections.namedtuple("FilterCase", "name map move x y z height_threshold bin_size marks")
Restated = collections.namedtuple("Restated", "keep key seconds")


def grid_of(case):
    """The oracle's grid of a filter case: (width, height, resolution) as the engine's create_map rounds them, moved."""
    import fdm_ref_py as R
    w, h, res = case.map
    grid = R.RefEngine(float(F32(w)), float(F32(h)), float(F32(res)))
    if case.move:
        grid.move(*case.move)
    return grid


def bin_of(case):
    """The bin size the filter uses (pcd_convert.cpp:308-309): 0 = the resolution."""
    return F32(case.bin_size) if case.bin_size > 0 else F32(case.map[2])


def cutoff_of_zero(bin_size, height_threshold):
    """The cutoff of a cell whose z_min is 0 and whose peak is bin 0, in fp32 as :219 and :257 compute it."""
    return F32(F32(F32(0.0) + F32(F32(F32(0.0) + F32(0.5)) * F32(bin_size))) + F32(height_threshold))


class _Builder:
    """Collects points cell by cell; `order()` shuffles the cloud but keeps every marked cell's points in the order they
    were given (the order a tie or a run is about)."""

    def __init__(self, grid, seed):
        self.grid, self.rng = grid, np.random.default_rng(seed)
        self.res = float(grid.geometry().resolution)
        self.pts, self.rank, self.tag, self.names = [], [], [], []

    def free(self, p):
        """Points (m, 3) at places of their own."""
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        self.pts.append(p)
        self.rank.append(self.rng.uniform(0.0, 1.0, len(p)))
        self.tag.append(np.full(len(p), -1))

    def cell(self, r, c, zs, mark=None, jitter=0.4):
        ok, (cx, cy) = self.grid.get_position(int(r), int(c))
        assert ok and self.grid.get_index(cx, cy) == (True, (int(r), int(c)))
        m, j = len(zs), jitter * self.res
        p = np.stack([cx + self.rng.uniform(-j, j, m), cy + self.rng.uniform(-j, j, m), np.asarray(zs, dtype=np.float64)], 1)
        self.pts.append(p)
        u = self.rng.uniform(0.0, 1.0, m)
        self.rank.append(np.sort(u) if mark else u)
        self.tag.append(np.full(m, len(self.names) if mark else -1))
        if mark:
            self.names.append(mark)

    def order(self, tail=()):
        p, rank, tag = np.concatenate(self.pts), np.concatenate(self.rank), np.concatenate(self.tag)
        o = np.argsort(rank, kind="stable")
        p, tag = p[o], tag[o]
        if len(tail):
            p = np.concatenate([p, np.asarray(tail, dtype=np.float64)])
            tag = np.concatenate([tag, np.full(len(tail), -1)])
        marks = {name: np.flatnonzero(tag == k) for k, name in enumerate(self.names)}
        return p[:, 0].astype(F32), p[:, 1].astype(F32), p[:, 2].astype(F32), marks


def _scene(b, rows, cols, n_cells, per_cell, skip=()):
    """Noisy ground in n_cells random cells of the map, a canopy 3 m up over half of them."""
    rng = b.rng
    ids = rng.permutation(rows * cols)
    ids = ids[~np.isin(ids, [r * cols + c for r, c in skip])][:n_cells]
    for k, i in enumerate(ids):
        z = rng.normal(0.0, 0.03, per_cell)
        if k % 2 == 0:
            z[: per_cell // 3] = rng.normal(3.0, 0.05, per_cell // 3)
        b.cell(i // cols, i % cols, z)


# ---- (a) the bin sort's passes ----
BIN_SIZES = {"bins_2": 0.1, "bins_3": 5e-4, "bins_4": 1e-6}
Z_SET = (0.0, 0.25, 12.5, 12.75, 49.9, 50.15)
BINS_HT = 2.0


@functools.lru_cache(maxsize=None)
def _bins_cloud():
    import fdm_ref_py as R
    grid = R.RefEngine(float(F32(26.0)), float(F32(26.0)), float(F32(0.1)))
    g = grid.geometry()
    assert (g.rows, g.cols) == (260, 260)
    b = _Builder(grid, 51)
    rng = b.rng
    corners = [0, 259, 259 * 260, 260 * 260 - 1]
    ids = rng.permutation(260 * 260)
    ids = ids[~np.isin(ids, corners)]
    for i in corners + list(ids[:1996]):                             # 2 000 cells of 10 points: 20 000
        b.cell(i // 260, i % 260, rng.choice(Z_SET, 10, p=(0.3, 0.2, 0.15, 0.15, 0.1, 0.1)))
    hand = iter(ids[1996:])

    def cell(zs, mark):
        i = next(hand)
        b.cell(i // 260, i % 260, zs, mark)

    cell([0.5, 0.5, 30.0, 30.0, 10.0], "tie_low_first")              # two equal peaks: the low one is the ground
    cell([30.0, 30.0, 0.5, 0.5, 10.0], "tie_high_first")
    for name, size in BIN_SIZES.items():                             # at the cutoff of this bin size, and an ulp above it
        c = cutoff_of_zero(size, BINS_HT)
        cell([0.0, 0.0, 0.0, c, np.nextafter(c, F32(9))], "cutoff_" + name)
    cell([7.0], "single")
    cell([2.5] * 7, "all_equal")
    cell([0.0] * 40 + [5.0] * 39, "majority_low")
    cell([1.0, 1.0, 20.0, 20.0, 40.0, 40.0], "three_peaks")
    cell([0.0, 30.0, 30.0, 30.0], "peak_high")
    cell([-50.15, -50.15, -0.25, 0.0], "negative")
    cell([0.25, 12.5, 12.5, 12.5, 12.75, 49.9], "peak_inside")
    out = b.order(tail=[[99.0, 0.0, 1.0], [0.0, -99.0, 1.0], [0.5, 0.5, np.nan], [-3.0, 2.0, np.nan]])
    return out


# ---- (b) the cell sort's passes ----
def _cells_1():
    c = FilterCase("cells_1", (1.5, 1.7, 0.1), None, None, None, None, 0.5, 0.0, None)
    b = _Builder(grid_of(c), 52)
    _scene(b, 15, 17, 250, 12)
    x, y, z, marks = b.order(tail=[[9.0, 0.0, 1.0], [0.0, 0.0, np.nan]])
    return c._replace(x=x, y=y, z=z, marks=marks)


CELLS_256_SKIPPED = 60


def _cells_256():
    """ncell = 256: the skip key needs the ninth bit.  Storage cell 0 holds five points at z = 0 early in the input, then
    come 60 points without a cell (30 outside the map, 30 with a NaN z over cell 0), then a thousand points 1 to 51 m
    up, two per bin: the ground peak is bin 0 and all thousand go.  A cell sort over eight bits files the skipped points
    under cell 0 between the five and the thousand; the thousand are then a run of their own whose head — done long after
    the head of the run of five — leaves the cutoff of ITS peak, bin 10, and a dozen of them stay."""
    c = FilterCase("cells_256", (1.6, 1.6, 0.1), None, None, None, None, 0.5, 0.0, None)
    grid = grid_of(c)
    rng = np.random.default_rng(53)

    def part(seed, n_cells, extra=None):
        b = _Builder(grid, seed)
        _scene(b, 16, 16, n_cells, 10, skip=[(0, 0)])
        if extra:
            extra(b)
        return b.order()

    ok, (cx, cy) = grid.get_position(0, 0)
    assert ok and grid.get_index(cx, cy) == (True, (0, 0))
    first = part(531, 70)
    b0 = _Builder(grid, 532)
    b0.cell(0, 0, [0.0] * 5, "cell0_early")
    early = b0.order()
    skipped = np.array([[40.0 + k, 0.0, 1.0] for k in range(CELLS_256_SKIPPED // 2)] +
                       [[cx, cy, np.nan]] * (CELLS_256_SKIPPED // 2))
    skipped = skipped[rng.permutation(len(skipped))]
    high = [1.0 + 0.1 * j + 0.05 for j in range(500) for _ in range(2)]
    rest = part(533, 130, lambda b: b.cell(0, 0, high, "cell0_high"))
    x, y, z = (np.concatenate([first[k], early[k], skipped[:, k].astype(F32), rest[k]]) for k in range(3))
    at = first[0].size
    marks = {"cell0_early": at + early[3]["cell0_early"], "skipped": at + 5 + np.arange(CELLS_256_SKIPPED),
             "cell0_high": at + 5 + CELLS_256_SKIPPED + rest[3]["cell0_high"]}
    return c._replace(x=x, y=y, z=z, marks=marks)


def _cells_4():
    c = FilterCase("cells_4", (409.7, 409.6, 0.1), None, None, None, None, 0.5, 0.0, None)
    b = _Builder(grid_of(c), 54)
    for r, col in ((0, 0), (0, 4095), (4096, 0), (4096, 4095)):      # the four corners of the map
        b.cell(r, col, [0.0, 0.01, 0.02, 3.0], jitter=0.3)
    _scene(b, 4097, 4096, 296, 10)
    x, y, z, marks = b.order(tail=[[900.0, 0.0, 1.0], [0.0, 0.0, np.nan]])
    return c._replace(x=x, y=y, z=z, marks=marks)


# ---- (c) k_hf_peak's serial walk ----
LONG_CELL, ONE_BIN_CELL = (10, 10), (20, 15)


def _long_run():
    """Cell (10, 10): 5 000 points over 410 bins of 1 cm — twelve in each of bins 0 .. 398, a hundred more in bin 5 and in
    bin 350 (112 each, the tied peak: bin 5 is the ground), the cell's minimum 0.0 and one point in each of bins
    399 .. 409.  Cell (20, 15): 1 025 points at one height.  2 000 points of other cells between them."""
    c = FilterCase("long_run", (4.0, 3.0, 0.1), None, None, None, None, 0.5, 0.01, None)
    b = _Builder(grid_of(c), 55)
    size = 0.01
    zs = [(j + 0.5) * size for j in range(399) for _ in range(12)] + [5.5 * size] * 100 + [350.5 * size] * 100
    zs += [0.0] + [(j + 0.5) * size for j in range(399, 410)]
    zs = np.array(zs)[b.rng.permutation(len(zs))]
    b.cell(*LONG_CELL, zs, "long")
    b.cell(*ONE_BIN_CELL, [1.0] * 1025, "one_bin")
    _scene(b, 40, 30, 200, 10, skip=[LONG_CELL, ONE_BIN_CELL])
    x, y, z, marks = b.order()
    # (the marked cells' points keep their order among themselves; among the others they are spread by the shuffle)
    return c._replace(x=x, y=y, z=z, marks=marks)


# ---- (d) tiles of 4 096 pairs ----
N_TILE_LARGE, N_TILE_LIVE = 600_001, 20_000


def _tile_large():
    """As large_tile_cloud() of tests/test_raster_gpu.py: every pair goes through both sorts (a point without a z gets
    the key ncell and bin 0), the restatement touches only the 20 000 with a z.  40 m of z over bins of 0.5 mm: 80 000
    bins, three passes of the bin sort."""
    rng = np.random.default_rng(56)
    x = rng.uniform(-2.0, 2.0, N_TILE_LARGE).astype(F32)
    y = rng.uniform(-1.5, 1.5, N_TILE_LARGE).astype(F32)
    z = np.full(N_TILE_LARGE, np.nan, dtype=F32)
    live = rng.choice(N_TILE_LARGE, N_TILE_LIVE, replace=False)
    z[live] = rng.choice([0.0, 0.25, 1.0, 40.0], N_TILE_LIVE, p=(0.5, 0.2, 0.2, 0.1)).astype(F32)
    return FilterCase("tile_large", (4.0, 3.0, 0.1), None, x, y, z, 0.5, 5e-4, {})


# ---- (e) a moved map ----
MOVE = (3.37, -2.21)


def _moved():
    c = FilterCase("moved", (TB.W, TB.H, TB.RES), MOVE, None, None, None, 2.0, 0.0, None)
    grid = grid_of(c)
    g = grid.geometry()
    assert g.start_row != 0 and g.start_col != 0
    b = _Builder(grid, 57)
    rng = b.rng
    n = 1500
    hand = ((0, 0), (39, 29), (int(g.start_row), int(g.start_col)), (int(g.start_row) - 1, int(g.start_col) - 1))

    def elsewhere(p):                                                # the hand-made cells hold their own points only
        p = p.astype(F32).astype(np.float64)
        return p[[grid.get_index(px, py)[1] not in hand for px, py in p[:, :2]]]

    b.free(elsewhere(np.stack([g.position_x + rng.uniform(-TB.W / 2, TB.W / 2, n),
                               g.position_y + rng.uniform(-TB.H / 2, TB.H / 2, n), rng.normal(0.0, 0.03, n)], 1)))
    b.free(elsewhere(np.stack([g.position_x + rng.uniform(-1.5, 0.5, 300), g.position_y + rng.uniform(-1.0, 1.0, 300),
                               rng.normal(3.0, 0.05, 300)], 1)))
    cut = cutoff_of_zero(TB.RES, 2.0)
    for r, col in hand:
        b.cell(r, col, [0.0] * 45 + [cut, np.nextafter(cut, F32(9)), 5.0], "moved_%d_%d" % (r, col))   # storage corners, the seam
    x, y, z, marks = b.order(tail=[[0.0, 0.0, 1.0], [g.position_x, g.position_y, np.nan]])   # the old centre: outside now
    return c._replace(x=x, y=y, z=z, marks=marks)


FILTER_CASES = ("bins_2", "bins_3", "bins_4", "cells_1", "cells_256", "cells_4", "long_run", "tile_large", "moved")
_FILTER_BUILDERS = {"cells_1": _cells_1, "cells_256": _cells_256, "cells_4": _cells_4, "long_run": _long_run,
                    "tile_large": _tile_large, "moved": _moved}


@functools.lru_cache(maxsize=None)
def filter_case(name):
    if name in BIN_SIZES:
        x, y, z, marks = _bins_cloud()
        c = FilterCase(name, (26.0, 26.0, 0.1), None, x, y, z, BINS_HT, BIN_SIZES[name], marks)
    else:
        c = _FILTER_BUILDERS[name]()
    for a in (c.x, c.y, c.z):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _cells_of(cloud):
    """floating_cells of a case's cloud (the three bins_* cases share one)."""
    c = filter_case("bins_2" if cloud == "bins" else cloud)
    key = DR.floating_cells(grid_of(c), c.x, c.y, c.z)
    key.setflags(write=False)
    return key


@functools.lru_cache(maxsize=None)
def restated_filter(name):
    """Restated(keep, key, seconds) of a filter case, read-only."""
    c = filter_case(name)
    t0 = time.perf_counter()
    key = _cells_of("bins" if name in BIN_SIZES else name)
    keep = DR.restate_floating_grouped(None, c.x, c.y, c.z, c.height_threshold, bin_of(c), key=key)
    keep.setflags(write=False)
    return Restated(keep, key, time.perf_counter() - t0)


def cell_key(r, c):
    return (int(r) << 32) | int(c)


def largest_bin(name):
    """The largest bin index of any point of the case, by the restatement's arithmetic: the key range of the bin sort."""
    c = filter_case(name)
    return int(DR.floating_bins(restated_filter(name).key, c.z, bin_of(c))[3].max())


def sort_passes(max_value):
    """Passes of the radix sort over keys 0 .. max_value: ceil(bits / 8), bits as fdm_rsort.hpp's rs_key_bits has them
    (at least 1, at most 32)."""
    bits = 1
    while bits < 32 and (int(max_value) >> bits) != 0:
        bits += 1
    return (bits + 7) // 8


# ---- (f) pipeline clouds ----
PipeCase = collections.namedtuple("PipeCase", "name cloud config sor_keeps_all")
BASE = dict(TB.CONFIG, method="mean")
N_SCAN_CHUNKS = 263_000


def _channels(rng, m):
    return {"intensity": rng.uniform(0, 1, m).astype(F32), "rgb": rng.integers(0, 1 << 24, m).astype(np.uint32)}


def _one_cell():
    rng = np.random.default_rng(61)
    z = np.concatenate([rng.normal(0.0, 0.05, 180), rng.normal(3.0, 0.05, 20)])[rng.permutation(200)]
    c = {"x": np.full(200, 1.25, dtype=F32), "y": np.full(200, -0.75, dtype=F32), "z": z.astype(F32)}
    return PipeCase("one_cell", dict(c, **_channels(rng, 200)), dict(BASE, inpaint_iterations=3), False)


def _one_row():
    rng = np.random.default_rng(62)
    z = np.concatenate([rng.normal(0.0, 0.02, 340), rng.normal(3.0, 0.05, 60)])
    y = np.concatenate([rng.uniform(-4.0, 4.0, 340), rng.uniform(-1.0, 1.0, 60)])
    o = rng.permutation(400)
    c = {"x": np.full(400, 2.5, dtype=F32), "y": y[o].astype(F32), "z": z[o].astype(F32)}
    return PipeCase("one_row", dict(c, **_channels(rng, 400)), dict(BASE, inpaint_iterations=3), False)


def _utm():
    c = TB.dem_cloud()
    shift = {"x": 5.0e5, "y": 4.9e6, "z": 150.0}
    c.update({k: (c[k].astype(np.float64) * 20.0 + s).astype(F32) for k, s in shift.items()})
    return PipeCase("utm", c, dict(BASE, resolution=2.0, inpaint_iterations=3), False)


def _scan_chunks():
    """263 000 points on 12 x 8 m: 1 028 blocks of 256 in the first compaction, which keeps every point, and more than
    1 024 in the second, which the height filter feeds with irregular counts (a canopy over a third of the area).

    Outlier removal with sor_std_mul = 1e9 keeps every point, shown without the k-NN search: the threshold is
    gm + 1e9 sd with sd^2 = sum (m_i - gm)^2 / n, so max m_i - gm <= sqrt(n) sd, far below 1e9 sd once sd > 0 — and
    sd > 0 unless all mean distances are equal, which those of 263 000 random points are not (the GPU test checks
    n_after_sor == n, the threshold only for being finite)."""
    rng = np.random.default_rng(63)
    n, nc = N_SCAN_CHUNKS, int(N_SCAN_CHUNKS * 0.15)
    x = np.concatenate([rng.uniform(-6.0, 6.0, n - nc), rng.uniform(-6.0, -2.0, nc)])
    y = rng.uniform(-4.0, 4.0, n)
    z = np.concatenate([0.1 * x[: n - nc] + rng.normal(0.0, 0.02, n - nc), rng.normal(3.0, 0.05, nc)])
    o = rng.permutation(n)
    c = {"x": x[o].astype(F32), "y": y[o].astype(F32), "z": z[o].astype(F32)}
    return PipeCase("scan_chunks", dict(c, **_channels(rng, n)), dict(BASE, sor_std_mul=1e9, inpaint_iterations=0), True)


def _none_survive(height_threshold, inpaint):
    """dem_cloud() under a threshold nothing passes: NaN (z <= NaN holds for no point) and -20 m (below every cell's
    minimum, the cloud being 15 m high at the most).  At -1 m — `minus_one_metre` — the reference still keeps 35 points:
    the ground below a canopy denser than itself, whose peak is the canopy's bin 3 m up; that case is compared like any
    other and is the smallest second compaction here."""
    name = "none_survive_%s_%d" % ("nan" if np.isnan(height_threshold) else "neg", inpaint)
    if height_threshold == -1.0:
        name = "minus_one_metre"
    return PipeCase(name, TB.dem_cloud(), dict(BASE, height_threshold=height_threshold, inpaint_iterations=inpaint), False)


def _refused_late():
    c = TB.dem_cloud()
    one = {"x": 0.5, "y": -0.5, "z": 3e9, "intensity": 0.5, "rgb": 7}
    c = {k: np.append(v, np.asarray(one[k], dtype=v.dtype)) for k, v in c.items()}
    return PipeCase("refused_late", c, dict(BASE, sor_std_mul=1e9, bin_size=1.0, inpaint_iterations=3), False)


FAR = np.array([[60, 55, 1], [-50, 40, 0], [45, -62, 2], [-58, -47, 0], [70, 3, 1], [2, 66, 0]], dtype=F32)


def _fallback():
    """dem_cloud() and six points 50 to 90 m away: the bounding box grows, with it the search grid's columns, and the six
    are further from their eighth neighbour than the rings reach: the brute-force queue of the outlier removal."""
    c = TB.dem_cloud()
    rng = np.random.default_rng(64)
    far = dict(zip("xyz", FAR.T), **_channels(rng, len(FAR)))
    c = {k: np.concatenate([v, far[k].astype(v.dtype)]) for k, v in c.items()}
    return PipeCase("fallback", c, dict(BASE, inpaint_iterations=3), False)


_PIPE_BUILDERS = {"one_cell": _one_cell, "one_row": _one_row, "utm": _utm, "scan_chunks": _scan_chunks,
                  "refused_late": _refused_late, "fallback": _fallback,
                  "minus_one_metre": lambda: _none_survive(-1.0, 3),
                  "none_survive_neg_0": lambda: _none_survive(-20.0, 0), "none_survive_neg_3": lambda: _none_survive(-20.0, 3),
                  "none_survive_nan_0": lambda: _none_survive(np.nan, 0), "none_survive_nan_3": lambda: _none_survive(np.nan, 3)}
NONE_SURVIVE = tuple(k for k in _PIPE_BUILDERS if k.startswith("none_survive"))
COMPARED = ("one_cell", "one_row", "utm", "fallback", "minus_one_metre") + NONE_SURVIVE   # (scan_chunks, refused_late: tests of their own)


@functools.lru_cache(maxsize=None)
def pipeline(name):
    p = _PIPE_BUILDERS[name]()
    for a in p.cloud.values():
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def restated_pipeline(name, floating="grouped"):
    """(DEM, seconds) of restate_build_dem; floating = "loop": with restate_floating, for the proof that the two agree."""
    import fdm_ref_py as R
    p = pipeline(name)
    c = p.cloud
    sor = (np.ones(c["x"].size, dtype=bool), None) if p.sor_keeps_all else None
    t0 = time.perf_counter()
    dem = DR.restate_build_dem(R, c["x"], c["y"], c["z"], c["intensity"], c["rgb"], sor=sor,
                               floating=DR.restate_floating if floating == "loop" else DR.restate_floating_grouped,
                               **p.config)
    seconds = time.perf_counter() - t0
    if dem is not None:
        for a in dem.store.values():
            a.setflags(write=False)
    return dem, seconds


def sor_must_queue(c, k, far):
    """How many of the points `far` of cloud c the ring search of the outlier removal cannot settle (the grid rule of
    tests/normal_cases.py's must_queue: a k-th neighbour further than (4 + 1/2) h, in a grid that goes on beyond ring 4
    around the point's column).  Sufficient, not necessary."""
    x, y, z = c["x"], c["y"], c["z"]
    h, gx, gy = DR.sor_grid(x.min(), y.min(), x.max(), y.max(), x.size, k)
    cx, cy = DR.knn_columns(x, x.min(), h, gx), DR.knn_columns(y, y.min(), h, gy)
    n = 0
    for q in far:
        d2 = ((x.astype(np.float64) - x[q]) ** 2 + (y.astype(np.float64) - y[q]) ** 2) + (z.astype(np.float64) - z[q]) ** 2
        d2[q] = np.inf
        kth = np.sqrt(np.sort(d2)[k - 1])
        covered = cx[q] - 4 <= 0 and cx[q] + 4 >= gx - 1 and cy[q] - 4 <= 0 and cy[q] + 4 >= gy - 1
        n += int(kth > 4.5 * float(h) and not covered)
    return n
