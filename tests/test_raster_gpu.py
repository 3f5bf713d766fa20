"""fromPointCloud / toPointCloud on the device (fastdem_amd/csrc/fdm_raster.hpp) against the NumPy restatement of
fastdem/src/pcd_convert.cpp (tests/raster_restate.py): every layer bit for bit — the NaN pattern identical, every other
value by its bits, `color` by bits — and the layer list in its order.  Per cell the reference applies Welford's update
in fp32 in INPUT order, so a walk in any other order shows in the variance's last bits (the run-length case).

Run on the GPU box:  python -m pytest tests -m gpu
"""
import functools

import numpy as np
import pytest

import raster_restate as RR
from helpers import assert_layers_bit_identical, lay_of

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H, RES = 4.0, 3.0, 0.1        # 40 x 30 cells


class RefMap:
    """The restated side: the oracle's grid for the cell of a point, the layers as NumPy arrays."""

    def __init__(self, R, width=W, height=H, res=RES, position=(0.0, 0.0), start=None):
        self.grid = R.RefEngine(float(F32(width)), float(F32(height)), float(F32(res)), position=position)
        if start:
            self.grid.set_start_index(*start)
        g = self.grid.geometry()
        self.order = list(RR.BASIC_LAYERS)
        self.store = {n: np.full((g.rows, g.cols), np.nan, dtype=F32) for n in self.order}

    def layers(self):
        return list(self.order)

    def layer(self, name):
        return self.store[name]

    def raster(self, c, method="max"):
        return RR.restate_raster(self.grid, self.store, self.order, c["x"], c["y"], c["z"], c.get("intensity"),
                                 c.get("rgb"), method)


def raster(eng, c, method="max"):
    return eng.from_point_cloud(c["x"], c["y"], c["z"], intensity=c.get("intensity"), rgb=c.get("rgb"), method=method)


def check(eng, ref):
    assert eng.layers() == ref.layers()
    assert_layers_bit_identical(eng, ref)


def uniform_cloud(n, seed, channels=True):
    rng = np.random.default_rng(seed)
    c = {"x": rng.uniform(-W / 2, W / 2, n).astype(F32), "y": rng.uniform(-H / 2, H / 2, n).astype(F32),
         "z": rng.normal(1.0, 0.5, n).astype(F32)}
    if channels:
        c["intensity"] = rng.uniform(0, 1, n).astype(F32)
        c["rgb"] = rng.integers(0, 1 << 24, n).astype(np.uint32)
    return c


# ---- the restated answers are computed once and shared by the fixture's two variants ----
@functools.lru_cache(maxsize=None)
def _count_case(n, method):
    import fdm_ref_py as R
    ref = RefMap(R)
    ref.raster(uniform_cloud(n, 100 + n, channels=(n % 2 == 1)), method)
    return ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_point_count_edges(gpu, R, n):
    c = uniform_cloud(n, 100 + n, channels=(n % 2 == 1))
    for method in RR.METHODS:
        ref = _count_case(n, method)
        eng = gpu.Engine.create_map(W, H, RES)
        rc, st = raster(eng, c, method)
        assert rc == 0 and st["n_points_used"] == int(ref.layer("n_points").sum()) >= n - 1
        assert st["n_cells_written"] == int((ref.layer("n_points") > 0).sum())
        check(eng, ref)
        eng.close()


N_LARGE_TILE = 600_001    # one past fdm_rsort.hpp's kRsSmallMax: tiles of 4 096 pairs, the histogram sized past the small tile's


def large_tile_cloud():
    """600 001 points of which 5 000, at random places of the input, have a z; the others' is NaN.  The device skips
    none of them before the sort (a skipped point gets the key ncell, behind every cell), so all 600 001 pairs go through
    the large-tile passes, and the walk has to find every cell's run in input order."""
    c = uniform_cloud(N_LARGE_TILE, 17)
    live = np.zeros(N_LARGE_TILE, dtype=bool)
    live[np.random.default_rng(18).choice(N_LARGE_TILE, 5000, replace=False)] = True
    c["z"][~live] = np.nan
    return c


@functools.lru_cache(maxsize=None)
def _large_tile_case():
    import fdm_ref_py as R
    c = large_tile_cloud()
    ref = RefMap(R)
    ref.raster(c, "mean")
    return c, ref


def test_large_tile_sort(gpu, R):
    """The 4 096-pair tile of the radix sort as fromPointCloud reaches it; `mean`: the variance shows a walk out of order."""
    c, ref = _large_tile_case()
    eng = gpu.Engine.create_map(W, H, RES)
    rc, st = raster(eng, c, "mean")
    assert rc == 0 and st["n_points_used"] == int(ref.layer("n_points").sum()) == 5000
    assert st["n_cells_written"] == int((ref.layer("n_points") > 0).sum()) > 1000
    check(eng, ref)
    eng.close()


RUNS = (1, 2, 63, 64, 65, 256, 257, 4000)


def run_length_cloud():
    """Chosen cells receive exactly RUNS points each, interleaved in input order with each other's and with 700 points of
    other cells; every cell's own points keep their relative order.  The 4 000-point cell's z are the order-sensitive
    values of tests/test_raster_restate.py."""
    rng = np.random.default_rng(5)
    cells = [(3 + 4 * k, 2 + 3 * k) for k in range(len(RUNS))]            # (row, col), unwrapped == buffer (start 0)
    per_cell = []
    for (r, c), m in zip(cells, RUNS):
        cx, cy = W / 2 - (r + 0.5) * RES, H / 2 - (c + 0.5) * RES
        z = RR.order_sensitive_values() if m == 4000 else rng.normal(2.0, 1.0, m).astype(F32)
        assert z.size == m
        per_cell.append((cx + rng.uniform(-0.04, 0.04, m), cy + rng.uniform(-0.04, 0.04, m), z))
    other = uniform_cloud(700, 6, channels=False)
    keep = np.array([(int((W / 2 - x) / RES), int((H / 2 - y) / RES)) not in set(cells)
                     for x, y in zip(other["x"], other["y"])])
    per_cell.append((other["x"][keep], other["y"][keep], other["z"][keep]))
    labels = np.concatenate([np.full(len(p[0]), k) for k, p in enumerate(per_cell)])
    rng.shuffle(labels)
    nxt = [0] * len(per_cell)
    x, y, z = (np.empty(labels.size, dtype=F32) for _ in range(3))
    for i, k in enumerate(labels):
        j = nxt[k]
        nxt[k] += 1
        x[i], y[i], z[i] = per_cell[k][0][j], per_cell[k][1][j], per_cell[k][2][j]
    c = {"x": x, "y": y, "z": z, "intensity": rng.uniform(0, 1, labels.size).astype(F32),
         "rgb": rng.integers(0, 1 << 24, labels.size).astype(np.uint32)}
    return c, cells


@functools.lru_cache(maxsize=None)
def _run_length_case():
    import fdm_ref_py as R
    c, cells = run_length_cloud()
    ref = RefMap(R)
    ref.raster(c, "mean")
    for (r, col), m in zip(cells, RUNS):
        assert ref.layer("n_points")[r, col] == m, (r, col, m)
    return c, ref


def test_run_length_edges_and_to_point_cloud(gpu, R):
    c, ref = _run_length_case()
    eng = gpu.Engine.create_map(W, H, RES)
    empty = eng.to_point_cloud()                                          # an untouched map: no point
    assert empty["x"].size == 0 and empty["intensity"] is None and empty["rgb"] is None
    rc, st = raster(eng, c, "mean")
    assert rc == 0 and st["n_cells_written"] == int((ref.layer("n_points") > 0).sum())
    check(eng, ref)
    check_cloud(eng.to_point_cloud(), RR.restate_to_cloud(ref.store, ref.grid.geometry()))


def check_cloud(got, want):
    assert got["x"].size == want["x"].size
    for k in ("x", "y", "z"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    for k in ("intensity", "rgb"):
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


def geometry_cloud(px, py):
    """Points on cell borders, on the inclusive upper map edge, just outside the lower one, and the non-finite ones."""
    rng = np.random.default_rng(9)
    res, hx, hy = np.float64(F32(RES)), np.float64(F32(W)) / 2, np.float64(F32(H)) / 2
    xs, ys = [], []
    for k in range(0, 41):                       # every row border (k = 0: the inclusive upper edge; 40: the lower one)
        xs.append(px + hx - k * res)
        ys.append(py + rng.uniform(-1.4, 1.4))
    for k in range(0, 31):
        xs.append(px + rng.uniform(-1.9, 1.9))
        ys.append(py + hy - k * res)
    xs += [px + hx, px - hx, px - hx - 1e-6, px + hx + 1e-6]          # corners and a hair beyond
    ys += [py + hy, py - hy, py, py]
    x = np.concatenate([np.array(xs, dtype=np.float64).astype(F32), (px + rng.uniform(-2.1, 2.1, 300)).astype(F32)])
    y = np.concatenate([np.array(ys, dtype=np.float64).astype(F32), (py + rng.uniform(-1.6, 1.6, 300)).astype(F32)])
    # one ulp either side of every border value too
    x = np.concatenate([x, np.nextafter(x[:41], F32(np.inf)), np.nextafter(x[:41], F32(-np.inf))])
    y = np.concatenate([y, y[:41], y[:41]])
    z = rng.normal(0.5, 0.2, x.size).astype(F32)
    n0 = x.size
    special = [(np.nan, py, 1.0), (px, np.nan, 1.0), (px, py, np.nan), (px + 0.31, py + 0.2, np.inf),
               (px - 0.52, py - 0.3, -np.inf), (px - 0.52, py - 0.3, 1.0), (np.inf, py, 1.0), (-np.inf, py, 1.0),
               (px + 0.31, py + 0.2, 2.0), (px + 0.73, py - 0.9, np.inf), (px + 0.73, py - 0.9, -np.inf)]
    sp = np.array(special, dtype=np.float64).astype(F32)
    x, y, z = np.concatenate([x, sp[:, 0]]), np.concatenate([y, sp[:, 1]]), np.concatenate([z, sp[:, 2]])
    order = np.random.default_rng(10).permutation(x.size)
    assert n0 + len(special) == x.size
    return {"x": x[order], "y": y[order], "z": z[order]}


@functools.lru_cache(maxsize=None)
def _geometry_case():
    import fdm_ref_py as R
    ref = RefMap(R, position=(3.3, -1.7), start=(17, 5))
    c = geometry_cloud(3.3, -1.7)
    ref.raster(c, "mean")
    return c, ref


def test_geometry_start_index_borders_and_non_finite_points(gpu, R):
    c, ref = _geometry_case()
    eng = gpu.Engine.create_map(W, H, RES)
    eng.set_start_index(17, 5)
    eng.set_position(3.3, -1.7)
    rc, st = raster(eng, c, "mean")
    assert rc == 0 and 0 < st["n_points_used"] < c["x"].size
    assert np.isinf(ref.layer("elevation_max")).any() and np.isnan(ref.layer("variance")[ref.layer("n_points") > 1]).any()
    check(eng, ref)
    check_cloud(eng.to_point_cloud(), RR.restate_to_cloud(ref.store, ref.grid.geometry()))


def test_channels(gpu, R):
    nan = np.nan
    # cell A: NaN intensity first (stays NaN); cell B: NaN later (ignored); cell C: equal intensities; colours: last wins
    pts = [(0.05, 0.05, 1.0, nan, 0x010203), (0.55, 0.05, 1.0, 0.3, 0x111111), (0.05, 0.06, 2.0, 0.9, 0x040506),
           (0.55, 0.06, 2.0, nan, 0x222222), (0.55, 0.07, 3.0, 0.2, 0xFFFFFFFF), (1.05, 0.05, 1.0, 0.5, 0x0000FF),
           (1.05, 0.06, 0.5, 0.5, 0x00FF00), (0.05, 0.07, 0.0, 0.95, 0x070809), (-1.05, -0.85, 4.0, -0.0, 0x0)]
    a = np.array(pts, dtype=np.float64)
    c = {"x": a[:, 0].astype(F32), "y": a[:, 1].astype(F32), "z": a[:, 2].astype(F32), "intensity": a[:, 3].astype(F32),
         "rgb": np.array([p[4] for p in pts], dtype=np.uint32)}
    eng, ref = gpu.Engine.create_map(W, H, RES), RefMap(R)
    assert raster(eng, c)[0] == 0
    ref.raster(c)
    assert np.isnan(ref.layer("intensity")[ref.grid.get_index(0.05, 0.05)[1]])
    check(eng, ref)
    # a cloud without either channel on a map that has both: the two layers keep every value
    plain = uniform_cloud(300, 31, channels=False)
    assert raster(eng, plain, "min")[0] == 0
    ref.raster(plain, "min")
    check(eng, ref)
    # only some valid cells have an intensity / a colour
    want = RR.restate_to_cloud(ref.store, ref.grid.geometry())
    assert want["intensity"] is not None and (want["intensity"] == 0).sum() > 100 and want["rgb"] is not None
    check_cloud(eng.to_point_cloud(), want)
    # intensity only
    eng2, ref2 = gpu.Engine.create_map(W, H, RES), RefMap(R)
    only = dict(plain, intensity=np.linspace(-1, 1, 300).astype(F32))
    assert raster(eng2, only)[0] == 0
    ref2.raster(only)
    check(eng2, ref2)
    assert "color" not in eng2.layers()
    check_cloud(eng2.to_point_cloud(), RR.restate_to_cloud(ref2.store, ref2.grid.geometry()))


def test_existing_content(gpu, R):
    a = uniform_cloud(1500, 41)
    b = uniform_cloud(900, 42)
    b["x"] = (np.abs(b["x"])).astype(F32)              # half of the map
    eng, ref = gpu.Engine.create_map(W, H, RES), RefMap(R)
    assert raster(eng, a, "mean")[0] == 0
    ref.raster(a, "mean")
    before = ref.layer("elevation").copy()
    assert raster(eng, b, "max")[0] == 0
    ref.raster(b, "max")
    same = before.view(np.uint32) == ref.layer("elevation").view(np.uint32)
    assert (same & np.isfinite(before)).sum() > 100 and (~same).sum() > 100   # cells B left alone, cells B took over
    check(eng, ref)


def scan(rng, n=900):
    return {"x": rng.uniform(-1.8, 1.8, n).astype(F32), "y": rng.uniform(-1.3, 1.3, n).astype(F32),
            "z": (rng.uniform(-0.3, 0.3, n) - 1.0).astype(F32)}


@pytest.mark.parametrize("held_back", [False, True])
@pytest.mark.parametrize("estimator", [0, 1])
def test_estimator_engine(gpu, R, estimator, held_back):
    """Record-backed fields are written in place, and a held-back update is not overtaken."""
    import torch
    from test_batch_gpu import T
    ce, cr = gpu.capi.default_config(), R.default_config()
    for cfg in (ce, cr):
        cfg.z_min, cfg.z_max, cfg.range_min, cfg.range_max = -3.0, 3.0, 0.0, 30.0
        cfg.estimation_type = estimator
    eng = gpu.Engine(W, H, RES, ce)
    ref = R.RefEngine(W, H, RES, cr)
    rng = np.random.default_rng(50 + estimator)
    Tbs, s0, s1 = T(0.0, 0.0, 1.0), scan(rng), scan(rng)
    if held_back:   # enqueue only: the scan's update is held back for the next launch
        d = [torch.from_numpy(s0[k]).cuda() for k in ("x", "y", "z")]
        eng.integrate_device(d[0], d[1], d[2], Tbs, T(0, 0))
    else:
        assert eng.integrate(s0["x"], s0["y"], s0["z"], Tbs, T(0, 0))[0] == 0
    assert ref.integrate(s0["x"], s0["y"], s0["z"], Tbs, T(0, 0))[0] == 0
    c = uniform_cloud(2000, 60 + estimator)
    assert raster(eng, c, "mean")[0] == 0
    order = ref.layers()
    store = {n: ref.layer(n) for n in order}
    written = RR.restate_raster(ref, store, order, c["x"], c["y"], c["z"], c["intensity"], c["rgb"], "mean")
    assert "variance" in written and "color" in written
    for n in written:
        ref.set_layer(n, store[n])
    assert eng.layers() == ref.layers()
    assert_layers_bit_identical(eng, ref)
    # the next scan carries intensity: on a record engine the rasterization created `intensity` as a plain array
    a1 = rng.uniform(0, 2, s1["x"].size).astype(F32)
    assert eng.integrate(s1["x"], s1["y"], s1["z"], Tbs, T(0.35, -0.2), intensity=a1)[0] == 0
    assert ref.integrate(s1["x"], s1["y"], s1["z"], Tbs, T(0.35, -0.2), intensity=a1)[0] == 0
    assert eng.layers() == ref.layers()
    assert_layers_bit_identical(eng, ref)


def test_nothing_lands(gpu, R):
    eng = gpu.Engine.create_map(W, H, RES)
    names = eng.layers()
    assert names == RR.BASIC_LAYERS
    z0 = np.zeros(0, F32)
    assert raster(eng, {"x": z0, "y": z0, "z": z0})[0] == gpu.capi.FDM_SKIP_EMPTY_CLOUD
    far = uniform_cloud(500, 71)
    far["x"] = far["x"] + F32(100.0)
    rc, st = raster(eng, far)
    assert rc == gpu.capi.FDM_SKIP_NO_CELL and st == {"n_points_used": 0, "n_cells_written": 0}
    nanz = uniform_cloud(500, 72)
    nanz["z"] = np.full(500, np.nan, dtype=F32)
    assert raster(eng, nanz)[0] == gpu.capi.FDM_SKIP_NO_CELL
    assert eng.layers() == names and not np.isfinite(eng.layer("elevation")).any()


def auto_clouds():
    rng = np.random.default_rng(80)
    big = {"x": rng.normal(12.0, 3.0, 5000).astype(F32), "y": rng.normal(-40.0, 2.0, 5000).astype(F32),
           "z": rng.normal(0.0, 1.0, 5000).astype(F32), "intensity": rng.uniform(0, 1, 5000).astype(F32)}
    big["x"][17] = np.nan           # a point without x does not stretch the box
    big["y"][18] = np.nan
    return [({"x": np.array([-5.0, 5.0, 0.0], F32), "y": np.array([-3.0, 3.0, 0.0], F32), "z": np.array([1.0, 2.0, 3.0], F32)}, 0.5),
            ({"x": np.array([-5.0, 5.0], F32), "y": np.array([-3.0, 3.0], F32), "z": np.array([1.0, 2.0], F32)}, 0.5),
            (big, 0.07)]


@functools.lru_cache(maxsize=None)
def _auto_case(k):
    import fdm_ref_py as R
    c, res = auto_clouds()[k]
    geo = RR.restate_auto_geometry(c["x"], c["y"], res)
    ref = RefMap(R, geo[0], geo[1], res, position=(geo[3], geo[4]))
    g = ref.grid.geometry()
    assert (g.length_x, g.length_y, g.resolution, g.rows, g.cols) == (geo[0], geo[1], geo[2], geo[5], geo[6])
    ref.raster(c, "max")
    return c, res, geo, ref


@pytest.mark.parametrize("k", [0, 1, 2])
def test_auto_size(gpu, R, k):
    c, res, geo, ref = _auto_case(k)
    eng = gpu.from_point_cloud(c["x"], c["y"], c["z"], res, intensity=c.get("intensity"), method="max")
    g = eng.geometry()
    assert (g.length_x, g.length_y, g.resolution, g.position_x, g.position_y, g.rows, g.cols) == geo
    assert (g.start_row, g.start_col) == (0, 0)
    check(eng, ref)
    if k == 2:      # the same from device arrays
        import torch
        d = {n: torch.from_numpy(v).cuda() for n, v in c.items()}
        eng2 = gpu.from_point_cloud(d["x"], d["y"], d["z"], res, intensity=d["intensity"])
        check(eng2, ref)


def test_auto_size_refusals(gpu):
    z0 = np.zeros(0, F32)
    assert gpu.from_point_cloud(z0, z0, z0, 0.5) is None
    one = np.ones(4, F32)
    with pytest.raises(gpu.EngineError):
        gpu.from_point_cloud(np.full(4, np.nan, F32), one, one, 0.5)
    with pytest.raises(gpu.EngineError):
        gpu.from_point_cloud(np.array([0, 1, np.inf, 2], F32), one, one, 0.5)


def test_tiled_engines_are_refused(gpu):
    cfg = gpu.capi.default_config()
    cfg.mode = gpu.capi.MODE_GLOBAL
    eng = gpu.Engine(W, H, RES, cfg, tile=(0, 0, 20, 30, 0, 0, 16, 30))
    c = uniform_cloud(100, 90)
    with pytest.raises(gpu.EngineError, match="tiled"):
        raster(eng, c)
    with pytest.raises(gpu.EngineError, match="tiled"):
        eng.to_point_cloud()
    st = gpu.capi.FdmRasterStats()
    assert gpu.capi.load().fdm_engine_from_point_cloud(eng._h, 0, None, None, None, None, None, 0, st) == gpu.capi.FDM_ERR_INVALID


def test_to_point_cloud_into_arrays_that_are_too_small(gpu):
    import ctypes as C
    eng = gpu.Engine.create_map(W, H, RES)
    assert raster(eng, uniform_cloud(300, 95, channels=False))[0] == 0
    x = np.full(4, 7.0, dtype=F32)
    n = C.c_uint64(0)
    rc = gpu.capi.load().fdm_engine_to_point_cloud(eng._h, 4, x.ctypes.data_as(C.c_void_p), None, None, None, None,
                                                   C.byref(n), None, None)
    assert rc == gpu.capi.FDM_SKIP_BUFFER_TOO_SMALL and n.value == eng.to_point_cloud()["x"].size > 4
    assert (x == 7.0).all()


def _same_bits(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same_bits(a[k], b[k], f"{what} {k}")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for k, (u, v) in enumerate(zip(a, b)):
            _same_bits(u, v, f"{what} [{k}]")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, what
        assert a.tobytes() == b.tobytes(), what
    else:
        assert a == b, what


def test_buffers_grow_from_a_small_call_to_a_larger_one(gpu):
    """The engine's on-demand buffers (message bytes, decoded channels, block counters, staged cloud, sort pairs and
    histograms, toPointCloud's channels, packed records of either kind) are sized by the first call with some slack.  One
    engine runs every call that owns one with a small input and then with one past that slack: 5, then 300 000 message
    points; 100, then 5 000 cloud points on a 64 x 64 map, which leave at most 100, then more than 2 000 valid cells
    for the three map-sized calls.  Each result equals the same call's on an engine that ran nothing before it (the larger
    cloud covers every cell of the smaller one, and a rasterized cell is overwritten whole: the maps are the same)."""
    import io_cases as K
    side = 6.4                                                            # 64 x 64 cells

    def cloud(n, seed):
        rng = np.random.default_rng(seed)
        return {"x": rng.uniform(-side / 2, side / 2, n).astype(F32), "y": rng.uniform(-side / 2, side / 2, n).astype(F32),
                "z": rng.normal(1.0, 0.5, n).astype(F32), "intensity": rng.uniform(0, 1, n).astype(F32),
                "rgb": rng.integers(0, 1 << 24, n).astype(np.uint32)}

    small, large = cloud(100, 71), cloud(5000, 72)
    large["x"][:100], large["y"][:100] = small["x"], small["y"]
    steps = ((small, "ingest_5", 5), (large, "ingest_300000", 300_000))
    valid = []
    eng = gpu.Engine.create_map(side, side, RES)
    for c, blob_name, n_msg in steps:
        fresh = gpu.Engine.create_map(side, side, RES)
        blob, lay = K.SCRATCH_BLOBS[blob_name]()
        _same_bits(eng.ingest_cloud2(blob, n_msg, lay_of(gpu, lay)), fresh.ingest_cloud2(blob, n_msg, lay_of(gpu, lay)),
                   blob_name)
        got, want = raster(eng, c, "mean"), raster(fresh, c, "mean")
        assert got == want and got[0] == 0, (got, want)
        assert eng.layers() == fresh.layers()
        assert_layers_bit_identical(eng, fresh)
        for call in ("to_point_cloud", "pack_cloud", "to_pcd"):
            _same_bits(getattr(eng, call)(), getattr(fresh, call)(), f"{call} after {c['x'].size} points")
        valid.append(eng.to_point_cloud()["x"].size)
        fresh.close()
    eng.close()
    assert valid[0] <= 100 and valid[1] > 2000, valid
