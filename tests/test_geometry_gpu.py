"""Map geometry against the oracle: odd-shaped, tiny, non-dyadic and far-off maps, and maps at the cell counts that
pick a pipeline — every layer bit for bit.

Why: the rest of the suite varies the SCANS around every pipeline threshold, but nearly always on a square map near the
world origin at 0.05 / 0.1 / 0.5 m.  Much of the device arithmetic depends on exactly what that leaves fixed: the
fixed-point index estimate `axis_fast` (fdm_device.hpp: fraction bits from max(rows, cols), error bound for small
|pos|), tile numbering `tile % tiles_r` in the record-pool and LDS-tiled stencil kernels, the float ray origin and the
per-ray quadrant sizes of the raycasting stage, the batch walker's rolling-window position, the egress cell centres, and
the cell-count rules of multi_run() (fdm_engine_multi.inl: kBatchMaxCells, kt >= 160 / 240).  A rows / cols swap, a
wrong size bound or an estimate that stops being "sure" far from the origin would show here.

  * GEOMETRIES: one seeded stream of a few hundred scans per map (sizes around the lowered pipeline thresholds, moves by
    fractions of a cell and by many cells on each axis, a jump beyond the shorter side, Kalman / P2, intensity / colour,
    raycasting, every entry point), obstacle + elevation behind every call, everything at the end, then every stencil
    kernel fdm_engine_post.inl dispatches to without a dbg_* option on the final map, and the packed cloud far out;
  * THRESHOLD_MAPS: short streams on 2^18 cells, one row more, kt = 160 (scans of 99 999 / 100 000 points) and kt = 240,
    with the path each scan must take written next to the rule of multi_run() it comes from;
  * a 1400 x 900 map 12 km out with two 1 M-point 128-beam scans and raycasting (record pools, k_ray_wedge);
  * uneven 2 x 2 spatial tiles of a GLOBAL map 25 / 41 km out against the whole map and the oracle;
  * test_geometry_table (no GPU): the table's claims and the oracle-only streams' non-vacuity.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from helpers import assert_arrays_close, assert_layers_bit_identical, pair, run_both, same_geometry
from test_batch_gpu import DeviceBatch, T

F32 = np.float32
TILED_MIN, VOXEL_SMALL_MAX, RAY_LARGE_MIN = 1500, 1100, 2600   # lowered as in test_long_horizon_gpu.py
LOCAL, GLOBAL = 0, 1
KALMAN, P2 = 0, 1
SENSOR_Z = 1.2

# id: (length_x, length_y, resolution, position, mode, (rows, cols), estimator, raycasting, intensity, colour, ground z,
#      scans, minimum of cells the oracle observes over the stream)
GEOMETRIES = {
    # neither side a multiple of 16 or 32, rows != cols
    "odd_tall": (3.7, 12.9, 0.1, (0.37, -1.23), LOCAL, (37, 129), KALMAN, True, True, False, 0.0, 220, 70000),
    # fewer rows than one tile, narrower than every stencil disc below
    "strip": (0.5, 40.0, 0.1, (0.0, 0.0), LOCAL, (5, 400), P2, False, False, False, 0.0, 200, 20000),
    # degenerate sizes: axis_fast is never "sure"
    "one_row": (0.1, 25.6, 0.1, (0.0, 0.0), GLOBAL, (1, 256), KALMAN, False, True, True, 0.0, 160, 4000),
    "two_by_three": (0.2, 0.3, 0.1, (0.0, 0.0), GLOBAL, (2, 3), P2, False, False, False, 0.0, 150, 150),
    # non-dyadic resolution
    "nondyadic": (14.1, 9.3, 0.15, (-2.2, 7.05), LOCAL, (94, 62), P2, True, True, True, 0.0, 220, 80000),
    # the float-promoted resolution the C++ API produces (0.07f)
    "float_res": (11.2, 17.5, float(np.float32(0.07)), (0.0, 0.0), LOCAL, (160, 250), KALMAN, False, True, False, 0.0,
                  200, 100000),
    # far from the origin, at altitude
    "far_local": (20.0, 12.0, 0.1, (31415.9, -27182.8), LOCAL, (200, 120), KALMAN, True, False, False, 1834.0, 220,
                  100000),
    # UTM-sized: float map-frame points are quantised to 0.5 m in y
    "utm_global": (30.0, 18.0, 0.2, (463217.0, 5319870.0), GLOBAL, (150, 90), P2, True, True, False, 312.0, 200, 70000),
    # points exactly on cell edges and on the border, representable in float; moves on rounding ties
    "dyadic_far_local": (16.0, 24.0, 0.125, (32768.0, -16384.0), LOCAL, (128, 192), KALMAN, True, False, False, 0.0, 200,
                         120000),
    "dyadic_far_global": (16.0, 24.0, 0.125, (32768.0, -16384.0), GLOBAL, (128, 192), P2, False, True, True, 0.0, 180,
                          120000),
}
DYADIC = ("dyadic_far_local", "dyadic_far_global")


def row(gid):
    (lx, ly, res, pos, mode, shape, est, ray, inten, colour, zg, n, min_cells) = GEOMETRIES[gid]
    return dict(lx=lx, ly=ly, res=res, pos=pos, mode=mode, shape=shape, est=est, ray=ray, inten=inten, colour=colour,
                zg=zg, n=n, min_cells=min_cells)


def cfg_of(g):
    def fill(c):
        c.z_min, c.z_max, c.range_min = -2.0, 4.0, 0.2
        c.range_max = float(min(40.0, 0.75 * max(g["lx"], g["ly"]) + 2.0))
        c.rc_log_odds_ghost, c.rc_clear_threshold, c.rc_height_conflict_threshold = 0.9, -0.5, 0.02
        c.mode, c.estimation_type, c.raycast_enabled = g["mode"], g["est"], int(g["ray"])
        return c
    return fill


class Stream:
    """The seeded call stream of one geometry (numpy Generator: the stream is the test's definition).  A call is
    (how, scans, poses, ray, phantom): how 0 = enqueue-only one scan per call, 1 = the synchronous host call for the
    first scan and a batch for the rest, else one batch call; phantom = a tall block written into the elevation layer
    before the call (on both sides) for the rays to clear."""

    def __init__(self, gid, seed):
        self.g = g = row(gid)
        self.gid = gid
        self.rng = np.random.default_rng(seed)
        self.px, self.py = g["pos"]
        self.k = 0
        self.dyadic = gid in DYADIC
        self.short, self.long = min(g["lx"], g["ly"]), max(g["lx"], g["ly"])
        self.jumps = {int(j) for j in self.rng.choice(np.arange(20, g["n"] - 20), 2, replace=False)}

    def size(self):
        r = self.rng
        pick = int(r.integers(0, 10))
        if pick < 3:
            return int(r.integers(1, 400))
        if pick < 5:   # around the sort-free voxel filter's limit
            return int(r.integers(VOXEL_SMALL_MAX - 150, VOXEL_SMALL_MAX + 150))
        if pick < 7:   # around the record-pool pipeline's threshold
            return int(r.integers(TILED_MIN - 200, TILED_MIN + 200))
        if pick < 9:   # around the sector-window walk's threshold
            return int(r.integers(RAY_LARGE_MIN - 300, RAY_LARGE_MIN + 300))
        return int(r.integers(3000, 6000))

    def yaw(self):
        return 0.0 if self.dyadic else 0.013 * self.k

    def pose(self):
        """Moves on one axis at a time: fractions of a cell, many cells, and (twice per stream) a jump longer than the
        map's shorter side but shorter than its longer side, along each axis in turn.  GLOBAL maps do not move: the
        robot stays on the map."""
        r, g = self.rng, self.g
        res = g["res"]
        axis = int(r.integers(0, 2))
        if self.k in self.jumps:
            d = float(r.choice([-1.0, 1.0])) * 0.5 * (self.short + self.long) if self.short < self.long else 1.2 * self.short
            axis = len([j for j in self.jumps if j <= self.k]) % 2
        elif int(r.integers(0, 6)) == 0:
            d = float(r.choice([-1.0, 1.0])) * float(r.integers(3, 25)) * res
        else:
            d = float(r.uniform(-0.6, 0.6)) * res
        if g["mode"] == GLOBAL:
            lim = 0.3 * (g["lx"] if axis == 0 else g["ly"])
            d = float(np.clip(d, -lim, lim))
        if self.dyadic:   # multiples of half a cell: moves on rounding ties, points on cell edges stay representable
            d = round(d / (res / 2)) * (res / 2)
        if g["mode"] == GLOBAL:
            cx, cy = g["pos"]
            nx, ny = (self.px + d, self.py) if axis == 0 else (self.px, self.py + d)
            if abs(nx - cx) > 0.45 * g["lx"] or abs(ny - cy) > 0.45 * g["ly"]:
                nx, ny = self.px - (d if axis == 0 else 0.0), self.py - (d if axis == 1 else 0.0)
            self.px, self.py = nx, ny
        elif axis == 0:
            self.px += d
        else:
            self.py += d
        self.k += 1
        return T(self.px, self.py, self.g["zg"], yaw=self.yaw())

    def cloud(self, n, Twb):
        """Points of the map around the robot (in world offsets, turned into the base frame), ground near the base."""
        r, g = self.rng, self.g
        res = g["res"]
        if g["mode"] == GLOBAL:
            cx, cy = g["pos"][0] - Twb[0, 3], g["pos"][1] - Twb[1, 3]
        else:
            cx = cy = 0.0
        hx, hy = g["lx"] / 2 + 2 * res, g["ly"] / 2 + 2 * res
        if self.dyadic:   # on the half-cell lattice: cell edges, cell centres, the border itself
            q = res / 2
            dx = r.integers(int(-hx / q), int(hx / q) + 1, n) * q + round(cx / q) * q
            dy = r.integers(int(-hy / q), int(hy / q) + 1, n) * q + round(cy / q) * q
            z = (r.integers(-16, 5, n) * (1.0 / 64.0) - SENSOR_Z).astype(F32)
        else:
            if int(r.integers(0, 3)) == 0:
                dx, dy = r.uniform(cx - hx, cx + hx, n), r.uniform(cy - hy, cy + hy, n)
            else:   # a patch: most tiles see nothing of this scan
                w = r.uniform(0.1, 0.35) * self.long
                px, py = r.uniform(cx - hx, cx + hx), r.uniform(cy - hy, cy + hy)
                dx, dy = r.uniform(px - w, px + w, n), r.uniform(py - w, py + w, n)
            z = (r.uniform(-0.5, 0.3, n) - SENSOR_Z).astype(F32)
        c, s = np.cos(-self.yaw()), np.sin(-self.yaw())
        x = (c * dx - s * dy).astype(F32)
        y = (s * dx + c * dy).astype(F32)
        kind = int(r.integers(0, 10))
        if kind == 0:
            z[::3] += F32(1.5)                  # tall things: obstacle cells, rays above the ground
        elif kind == 1:
            z[::5] = F32(-SENSOR_Z)             # map-frame heights exactly at the ground (+0.0 / -0.0 at zg = 0)
        elif kind == 2 and n > 20:
            x[n // 2:], y[n // 2:], z[n // 2:] = x[0], y[0], z[0]   # exact duplicates
        out = {"x": x, "y": y, "z": z, "intensity": None, "rgb": None}
        if g["inten"] and int(r.integers(0, 4)) != 0:
            out["intensity"] = r.uniform(0, 1, n).astype(F32)
        if g["colour"] and out["intensity"] is not None:
            out["rgb"] = r.integers(0, 1 << 24, n, dtype=np.uint32)
        return out

    def calls(self):
        r, g = self.rng, self.g
        done = 0
        while done < g["n"]:
            count = int(r.integers(1, 20))
            how = int(r.integers(0, 6))
            ray = g["ray"] and int(r.integers(0, 4)) != 0
            phantom = g["ray"] and int(r.integers(0, 12)) == 0
            poses, scans = [], []
            for _ in range(count):
                poses.append(self.pose())
                scans.append(self.cloud(self.size(), poses[-1]))
            # one call keeps its optional channels (a batch is one layout); the stream changes them between calls
            for s in scans[1:]:
                for ch in ("intensity", "rgb"):
                    if (s[ch] is None) != (scans[0][ch] is None):
                        s[ch] = None if scans[0][ch] is None else (
                            r.uniform(0, 1, s["x"].size).astype(F32) if ch == "intensity"
                            else r.integers(0, 1 << 24, s["x"].size, dtype=np.uint32))
            done += count
            yield how, scans, poses, ray, phantom


TBS = T(0.0, 0.0, SENSOR_Z)


def phantom_block(ref, rng):
    a = ref.layer("elevation").copy()
    r0, c0 = int(rng.integers(0, max(1, a.shape[0] - 6))), int(rng.integers(0, max(1, a.shape[1] - 6)))
    zg = float(np.nanmedian(a)) if np.isfinite(a).any() else 0.0
    a[r0:r0 + 6, c0:c0 + 6] = F32(zg + 1.25)
    return a


def set_ray(o, ray):
    c = o.cfg
    c.raycast_enabled = int(ray)
    o.set_config(c)


def oracle_scans(ref, scans, poses, tally):
    rc = st = None
    for s, Twb in zip(scans, poses):
        kw = {c: s[c] for c in ("intensity", "rgb") if s[c] is not None}
        rc, st = ref.integrate(s["x"], s["y"], s["z"], TBS, Twb, **kw)
        tally["cells"] += st["n_cells_touched"]
        if ref.cfg.raycast_enabled and rc == 0:
            tally["cleared"] += ref.last_ray_stats()["n_cleared"]
    return rc, st


def run_oracle_stream(R, gid, seed=1):
    """The stream on the oracle alone: (oracle, tally of observed / cleared cells)."""
    g = row(gid)
    cr = cfg_of(g)(R.default_config())
    ref = R.RefEngine(g["lx"], g["ly"], g["res"], cr, position=g["pos"])
    st = Stream(gid, seed)
    tally = {"cells": 0, "cleared": 0}
    for how, scans, poses, ray, phantom in st.calls():
        set_ray(ref, ray)
        if phantom and ref.exists("elevation"):
            ref.set_layer("elevation", phantom_block(ref, st.rng))
        oracle_scans(ref, scans, poses, tally)
    return ref, tally


# ------------------------------------------------------------------ 3: cell-count thresholds ----
# id: (length_x, length_y, rows, cols, scan sizes of the stream)
THRESHOLD_MAPS = {
    "cells_2p18": (51.2, 51.2, 512, 512, (600, 5000)),          # exactly kBatchMaxCells: batches allowed, kt = 256
    "cells_2p18_plus_row": (51.3, 51.2, 513, 512, (600, 5000)),  # one row over kBatchMaxCells: never a batch
    "kt160": (40.0, 41.0, 400, 410, (99999, 100000)),           # kt = 160: record pools only from 100 000 points
    "kt240": (48.0, 51.2, 480, 512, (600, 5000)),               # kt = 240: record pools from tiled_min (2 048) points
}
K_BATCH_MAX_CELLS = 1 << 18
DEFAULT_TILED_MIN = 2048


def expected_path(rows, cols, n):
    """(record-pool pipeline?, may ride in a batch?) of an n-point scan on a rows x cols map, engine defaults — the
    rules of multi_run() and enqueue_scan, restated so that a change to them fails here loudly."""
    ncell = rows * cols
    kt = ncell // 1024                                       # `kt = e->ncell / 1024u`
    enough_tiles = kt >= 240 or (kt >= 160 and n >= 100000)  # `enough_tiles = ... kt >= 240 || (kt >= 160 && s.n >= 100000)`
    tiled = n >= DEFAULT_TILED_MIN and enough_tiles          # `e->tiled && s.n >= e->tiled_min && enough_tiles`: breaks the run
    batch = ncell <= K_BATCH_MAX_CELLS and not tiled         # `e->ncell > kBatchMaxCells` -> no batch at all
    return tiled, batch


# ================================================================== 6: the table, without a GPU ====
def test_geometry_table(R):
    for gid in GEOMETRIES:
        g = row(gid)
        ref = R.RefEngine(g["lx"], g["ly"], g["res"], position=g["pos"])
        assert (ref.rows, ref.cols) == g["shape"], (gid, ref.rows, ref.cols)
        geo = ref.geometry()
        assert (geo.position_x, geo.position_y) == tuple(float(v) for v in g["pos"]), gid
    assert all(r % 16 and c % 16 for r, c in (GEOMETRIES[k][5] for k in ("odd_tall", "nondyadic")))
    assert GEOMETRIES["odd_tall"][5][0] % 32 and GEOMETRIES["odd_tall"][5][1] % 32
    assert GEOMETRIES["strip"][5][0] < 16 and GEOMETRIES["one_row"][5][0] == 1
    assert GEOMETRIES["float_res"][2] != 0.07 and F32(GEOMETRIES["float_res"][2]) == F32(0.07)
    assert 2 * sum(GEOMETRIES[k][7] for k in GEOMETRIES) >= len(GEOMETRIES)
    assert GEOMETRIES["far_local"][7] and GEOMETRIES["utm_global"][7]
    # UTM northing: float map-frame points are quantised to 0.5 m
    assert np.spacing(F32(GEOMETRIES["utm_global"][3][1])) == F32(0.5)
    # dyadic_far: the position, the cell edges and the half-cell lattice are exact in float
    pos = GEOMETRIES["dyadic_far_local"][3]
    assert all(float(F32(p + 0.0625 * k)) == p + 0.0625 * k for p in pos for k in (-200, -1, 1, 200))
    # the threshold maps: cell counts and kt
    for tid, (lx, ly, rows, cols, sizes) in THRESHOLD_MAPS.items():
        ref = R.RefEngine(lx, ly, 0.1)
        assert (ref.rows, ref.cols) == (rows, cols), tid
    assert 512 * 512 == K_BATCH_MAX_CELLS and 513 * 512 > K_BATCH_MAX_CELLS
    assert (400 * 410) // 1024 == 160 and (480 * 512) // 1024 == 240
    assert expected_path(400, 410, 99999) == (False, True) and expected_path(400, 410, 100000) == (True, False)
    assert expected_path(513, 512, 600) == (False, False) and expected_path(512, 512, 5000) == (True, False)
    # every stream observes what it is there for (on the oracle alone)
    for gid in GEOMETRIES:
        g = row(gid)
        _, tally = run_oracle_stream(R, gid)
        assert tally["cells"] >= g["min_cells"], (gid, tally)
        if g["ray"]:
            assert tally["cleared"] > 0, (gid, tally)


# ================================================================== 1 + 2: streams, stencils, egress ====
def compare(eng, ref, what, names=None):
    eng.sync()
    assert sorted(eng.layers()) == sorted(ref.layers()), (what, eng.layers(), ref.layers())
    assert_layers_bit_identical(eng, ref, names=names)
    assert same_geometry(eng.geometry(), ref.geometry()), what


def both(objs, fn):
    return [fn(o) for o in objs]


def exact(eng, ref, names):
    for n in names:
        assert_arrays_close(eng.layer(n), ref.layer(n), n, 0.0, 0.0)


def stencils(gpu, R, eng, ref, res, small):
    """Every stencil kernel fdm_engine_post.inl reaches without a dbg_* option, on the final map of a stream."""
    rng = np.random.default_rng(5)
    el = ref.layer("elevation").copy()
    holes = ~np.isfinite(el)
    fill = (0.3 * np.sin(np.arange(el.size) * 0.37).reshape(el.shape) + float(np.nanmean(el)) if (~holes).any() else 0.0)
    el = np.where(holes & (rng.uniform(size=el.shape) < 0.6), fill, el).astype(F32)   # dense enough for the discs
    half = np.abs(rng.normal(0.05, 0.03, el.shape)).astype(F32) + F32(0.005)
    both((eng, ref), lambda o: (o.set_layer("elevation", el), o.set_layer("upper_bound", el + half),
                                o.set_layer("lower_bound", el - half)))
    # fusion: discs of 9 / 29 cells (k_fusion_f64_tiled<9> / <29>), 1 cell (<29, false>), quantile 0 on 29 cells
    # (k_fusion_net32_tiled), 37 and 325 cells (k_fusion_wave), > 1024 cells on the small maps (k_fusion_big)
    fus = [(1.5, 0.01, 0.99), (3.05, 0.01, 0.99), (0.9, 0.01, 0.99), (3.05, 0.0, 0.99), (3.3, 0.05, 0.95),
           (10.05, 0.01, 0.99)]
    if small:
        fus.append((18.6, 0.05, 0.95))
    for k, ql, qu in fus:
        both((eng, ref), lambda o: (o.set_layer("upper_bound", el + half), o.set_layer("lower_bound", el - half),
                                    o.apply_uncertainty_fusion(True, k * res, 2.0 * res, ql, qu, 1)))
        exact(eng, ref, ["upper_bound", "lower_bound"])
    # inpainting (k_inpaint_pass_tiled), median 3 / 5 / 17 (k_median3_tiled, k_median, k_median_sel)
    both((eng, ref), lambda o: o.apply_inpainting(3, 2))
    exact(eng, ref, ["elevation_inpainted"])
    for k, mv in ((3, 3), (5, 5), (17, 20)):
        both((eng, ref), lambda o: (o.set_layer("elevation", el), o.apply_spatial_smoothing("elevation", k, mv)))
        exact(eng, ref, ["elevation"])
    # features: 29-cell disc (k_features_tiled<2,3>), 113 cells (<6,7>), 113 cells at (0.3, 0.7) (k_features_sel)
    R.set_trig_mode(1)
    try:
        for k, lo, hi in ((3.05, 0.05, 0.95), (6.05, 0.05, 0.95), (6.05, 0.3, 0.7)):
            both((eng, ref), lambda o: (o.set_layer("elevation", el), o.apply_feature_extraction(k * res, 2, lo, hi)))
            exact(eng, ref, ["step", "slope", "roughness", "curvature", "_normal_x", "_normal_y", "_normal_z"])
    finally:
        R.set_trig_mode(0)


def disc_cells(radius_cells):
    k = int(np.floor(radius_cells + 1e-4))
    d = np.arange(-k, k + 1)
    return int(((d[:, None] ** 2 + d[None, :] ** 2) <= radius_cells ** 2 * (1 + 1e-5)).sum())


def test_stencil_discs_of_the_table():
    """The radii stencils() uses, in cells, hit the disc sizes that pick each kernel (CPU check)."""
    assert [disc_cells(k) for k in (0.9, 1.5, 3.05, 3.3, 6.05, 10.05)] == [1, 9, 29, 37, 113, 325]
    assert disc_cells(18.6) > 1024


@pytest.mark.gpu
@pytest.mark.parametrize("gid", sorted(GEOMETRIES))
def test_stream_on_the_geometry(gpu, R, gid):
    g = row(gid)
    eng, ref = pair(gpu, R, g["lx"], g["ly"], g["res"], cfg_of(g), position=g["pos"])
    assert (eng.rows, eng.cols) == g["shape"]
    default_variant = "tiled_min" not in gpu.Engine.default_options
    if default_variant:
        eng.set_option("tiled_min", TILED_MIN)
        eng.set_option("ray_large_min", RAY_LARGE_MIN)
    eng.set_option("voxel_small_max", VOXEL_SMALL_MAX)
    eng.enable_cell_ids(False)
    st = Stream(gid, 1)
    tally = {"cells": 0, "cleared": 0}
    launches0 = sum(eng.batch_launches())
    rc_r = st_r = None
    keep = []
    for ncall, (how, scans, poses, ray, phantom) in enumerate(st.calls()):
        both((eng, ref), lambda o: set_ray(o, ray))
        if phantom and ref.exists("elevation"):
            a = phantom_block(ref, st.rng)
            both((eng, ref), lambda o: o.set_layer("elevation", a))
        what = f"{gid}: call {ncall} (how {how}, {len(scans)} scans, ray {ray})"
        if how == 1:   # the synchronous host call, cell ids on, then the rest as a batch
            eng.enable_cell_ids(True)
            rc_r, st_r = run_both(eng, ref, scans[0], TBS, poses[0])
            eng.enable_cell_ids(False)
            tally["cells"] += st_r["n_cells_touched"]
            if ray and rc_r == 0:
                tally["cleared"] += ref.last_ray_stats()["n_cleared"]
            scans, poses = scans[1:], poses[1:]
        if scans:
            rc_r, st_r = oracle_scans(ref, scans, poses, tally)
            b = DeviceBatch(gpu, scans, TBS, poses)
            keep.append(b)
            if how == 0:   # enqueue-only, one scan per call
                for k in range(len(scans)):
                    assert eng.integrate_device_batch((gpu.capi.FdmDeviceScan * 1)(b.arr[k])) == 0
            else:
                assert eng.integrate_device_batch(b.arr) == 0
        compare(eng, ref, what, names=[n for n in ("obstacle", "elevation") if ref.exists(n)])
        assert eng.last_stats() == (rc_r, st_r), (what, eng.last_stats(), rc_r, st_r)
        keep.clear()
    compare(eng, ref, f"{gid}: at the end")
    assert tally["cells"] >= g["min_cells"], (gid, tally)
    if g["ray"]:
        assert tally["cleared"] > 0, (gid, tally)
    if default_variant and g["shape"][0] * g["shape"][1] <= K_BATCH_MAX_CELLS:
        assert sum(eng.batch_launches()) > launches0, f"{gid}: no batch launch in the whole stream"
    # the stencils on the final map
    for o in (eng, ref):
        set_ray(o, False)
    stencils(gpu, R, eng, ref, g["res"], small=g["shape"][0] * g["shape"][1] <= 20000)
    # egress: cell centres far from the origin
    if gid in ("far_local", "utm_global"):
        fe, se, de = eng.pack_cloud()
        fr, sr, dr = ref.pack_cloud()
        assert (fe, se) == (fr, sr) and de.shape == dr.shape and de.shape[0] > 0
        assert np.array_equal(de.view(np.uint32), dr.view(np.uint32)), gid


# ================================================================== 3: cell-count thresholds ====
def ground_cloud(rng, n, lx, ly):
    return {"x": rng.uniform(-lx / 2 - 0.5, lx / 2 + 0.5, n).astype(F32),
            "y": rng.uniform(-ly / 2 - 0.5, ly / 2 + 0.5, n).astype(F32),
            "z": (rng.uniform(-0.4, 0.6, n) - SENSOR_Z).astype(F32),
            "intensity": rng.uniform(0, 1, n).astype(F32), "rgb": None}


@pytest.mark.gpu
@pytest.mark.parametrize("tid", sorted(THRESHOLD_MAPS))
def test_cell_count_thresholds(gpu, R, tid):
    """Six batch calls on a map at a cell-count rule of multi_run(); the path of each call's last scan is the one
    expected_path() derives from the rules (default variant), and every layer matches the oracle bit for bit."""
    lx, ly, rows, cols, (small, big) = THRESHOLD_MAPS[tid]

    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 4.0, 0.2, 40.0
        c.mode, c.estimation_type, c.raycast_enabled = LOCAL, KALMAN, 0
        return c
    eng, ref = pair(gpu, R, lx, ly, 0.1, fill)
    assert (eng.rows, eng.cols) == (rows, cols)
    eng.enable_cell_ids(False)   # (an engine that owes cell ids takes no batch launch)
    default_variant = "tiled_min" not in gpu.Engine.default_options
    rng = np.random.default_rng(rows * 7 + cols)
    calls = [[small], [small] * 4, [big], [small] * 3 + [big], [big] * 2, [small] * 3]
    launches0 = sum(eng.batch_launches())
    x0 = 0.0
    for ncall, sizes in enumerate(calls):
        scans = [ground_cloud(rng, n, lx, ly) for n in sizes]
        poses = []
        for _ in sizes:
            x0 += 0.23
            poses.append(T(x0, -0.5 * x0, 0.0, yaw=0.01 * x0))
        before = sum(eng.batch_launches())
        b = DeviceBatch(gpu, scans, TBS, poses)
        assert eng.integrate_device_batch(b.arr) == 0
        rc_r, st_r = oracle_scans(ref, scans, poses, {"cells": 0, "cleared": 0})
        assert eng.last_stats() == (rc_r, st_r), (tid, ncall)
        compare(eng, ref, f"{tid}: call {ncall}")
        if not default_variant:
            continue
        tiled, batch = expected_path(rows, cols, sizes[-1])
        assert eng.last_pipeline() == int(tiled), (tid, ncall, sizes[-1])
        if not batch:   # a record-pool scan, or a map over kBatchMaxCells: the single-scan path
            assert eng.last_batch() == 0, (tid, ncall)
        if ncall == 1:  # four eligible scans behind one on the same pipeline: one batch launch takes them
            assert (eng.last_batch() >= 2) == batch, (tid, eng.last_batch())
            assert (sum(eng.batch_launches()) > before) == batch, tid
    if default_variant and rows * cols > K_BATCH_MAX_CELLS:
        assert sum(eng.batch_launches()) == launches0, f"{tid}: a batch launch on a map over kBatchMaxCells"


# ================================================================== 4: a large scan far out ====
@pytest.mark.gpu
def test_large_scans_on_a_far_non_square_map(gpu, R):
    """70 x 45 m @ 0.05 (1400 x 900 cells: the last 32-column tile is partial) in LOCAL mode 12 km / -8.5 km out, three
    128-beam scans of 1 M points with raycasting, the sensor 4 m inside a short edge: the record-pool update and the
    sector-window ray walk (k_ray_wedge).  Every layer bit for bit, cell ids too."""
    from fastdem_amd.synth import _lidar_scan, rot_z, translate

    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 5.0, 0.5, 40.0
        c.mode, c.estimation_type, c.sensor_type, c.raycast_enabled = LOCAL, KALMAN, 1, 1
        c.rc_log_odds_ghost, c.rc_clear_threshold, c.rc_height_conflict_threshold = 0.9, -0.5, 0.02
        return c
    eng, ref = pair(gpu, R, 70.0, 45.0, 0.05, fill, position=(12000.0, -8500.0))
    assert (eng.rows, eng.cols) == (1400, 900)
    rng = np.random.default_rng(44)
    Tbs = translate(-31.0, 0.0, 1.8)
    cleared = 0
    for k in range(3):
        s = _lidar_scan(rng, 128, -22.5, 22.5, 8192, translate(0.35 * k, 0.0, 1.8), 28.0, "azimuth")
        assert s["x"].size >= 1 << 20
        Twb = translate(12000.0 + 0.35 * k, -8500.0 - 0.12 * k, 0.0) @ rot_z(np.deg2rad(0.3) * k)
        if k == 1:   # a phantom wall in the sensor's view for the rays to clear
            a = ref.layer("elevation").copy()
            a[50:90, 300:600] = F32(1.5)
            both((eng, ref), lambda o: o.set_layer("elevation", a))
        run_both(eng, ref, s, Tbs, Twb)
        cleared += ref.last_ray_stats()["n_cleared"]
        compare(eng, ref, f"scan {k}")
    assert cleared > 0
    if "tiled_min" not in gpu.Engine.default_options:
        assert eng.last_pipeline() == 1


# ================================================================== 5: uneven spatial tiles far out ====
@pytest.mark.gpu
def test_uneven_halo_tiles_far_from_the_origin(gpu, R):
    """A GLOBAL map of 157 x 203 cells 25 / 41 km out, split 2 x 2 at row 70 and column 120, each tile with a 6-cell halo:
    the same scans into every tile, the whole map and the oracle, then the stencils.  The whole map equals the oracle
    bit for bit; the owned cells of every tile equal the whole map."""
    W, H, RES, HALO, POS = 15.7, 20.3, 0.1, 6, (-25000.0, 41000.0)

    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 4.0, 0.2, 30.0
        c.mode, c.estimation_type, c.raycast_enabled = GLOBAL, P2, 0
        return c
    whole, ref = pair(gpu, R, W, H, RES, fill, position=POS)
    whole.enable_cell_ids(False)
    rows, cols = whole.rows, whole.cols
    assert (rows, cols) == (157, 203)
    tiles = []
    for o_r0, o_r1 in ((0, 70), (70, rows)):
        for o_c0, o_c1 in ((0, 120), (120, cols)):
            s_r0, s_c0 = max(0, o_r0 - HALO), max(0, o_c0 - HALO)
            s_r1, s_c1 = min(rows, o_r1 + HALO), min(cols, o_c1 + HALO)
            t = gpu.Engine(W, H, RES, fill(gpu.capi.default_config()), position=POS,
                           tile=(s_r0, s_c0, s_r1 - s_r0, s_c1 - s_c0, o_r0, o_c0, o_r1 - o_r0, o_c1 - o_c0))
            tiles.append((t, (s_r0, s_r1, s_c0, s_c1), (o_r0, o_r1, o_c0, o_c1)))
    rng = np.random.default_rng(57)
    for k in range(8):
        px, py = POS[0] + rng.uniform(-4, 4), POS[1] + rng.uniform(-6, 6)
        s = ground_cloud(rng, int(rng.integers(3000, 30000)), W, H)
        s["x"] += F32(POS[0] - px)
        s["y"] += F32(POS[1] - py)
        Twb = T(px, py, 0.0, yaw=0.2 * k)
        c, sn = np.cos(-0.2 * k), np.sin(-0.2 * k)
        s["x"], s["y"] = (c * s["x"] - sn * s["y"]).astype(F32), (sn * s["x"] + c * s["y"]).astype(F32)
        kw = {"intensity": s["intensity"]}
        for o in [whole, ref] + [t for t, _, _ in tiles]:
            o.integrate(s["x"], s["y"], s["z"], TBS, Twb, **kw)
    compare(whole, ref, "after the scans")
    # a tile updates its owned window only: the halo ring is refreshed from the owners (a host-side halo exchange)
    for name in ref.layers():
        owned = np.full((rows, cols), np.nan, dtype=F32)
        for t, (a, b, c, d), (oa, ob, oc, od) in tiles:
            if t.exists(name):
                owned[oa:ob, oc:od] = t.layer(name)[oa - a:ob - a, oc - c:od - c]
        for t, (a, b, c, d), _ in tiles:
            if t.exists(name):
                t.set_layer(name, owned[a:b, c:d])

    def run(o):
        o.apply_uncertainty_fusion(True, 0.6, 0.2, 0.05, 0.95, 3)   # 6 cells
        o.apply_inpainting(3, 2)                                    # 3 cells
        o.apply_spatial_smoothing("elevation_inpainted", 5, 5)      # 2 cells
        o.apply_feature_extraction(0.6, 4, 0.05, 0.95)              # 6 cells
    R.set_trig_mode(1)
    try:
        for o in [whole, ref] + [t for t, _, _ in tiles]:
            run(o)
    finally:
        R.set_trig_mode(0)
    compare(whole, ref, "after the stencils")
    for name in ref.layers():
        full = whole.layer(name)
        for t, (a, b, c, d), (oa, ob, oc, od) in tiles:
            want = full[oa:ob, oc:od]
            if not t.exists(name):   # a tile no point with the channel landed in
                assert np.isnan(want).all(), name
                continue
            got = t.layer(name)[oa - a:ob - a, oc - c:od - c]
            assert_arrays_close(got, want, name, 0.0, 0.0)
