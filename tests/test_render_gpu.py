"""Layer -> RGBA image on the device (fdm_engine_render_layer, fastdem_amd/csrc/fdm_render.hpp) against a NumPy
restatement of fastdem::io::savePng's pixels (fastdem/src/io_png.cpp): computeRange (:32-65), the three colour
functions (:67-113) and the pixel loop (:128-171), written operation by operation in np.float32.  Pixels and the
returned range are compared EXACTLY.  (The sign of a selected zero is unspecified — std::nth_element and a radix
select may pick either of two equal elements — and cannot change a pixel: the range is compared with ==.)"""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_layers_bit_identical, pair, run_both, same_geometry

pytestmark = pytest.mark.gpu
F = np.float32
NORMALIZE = ("min_max", "percentile_1_99", "fixed_range")
COLORMAP = ("grayscale", "viridis", "jet")
FIXED = (-0.25, 0.4)
# the reference's eight viridis control colours (the contract, like the config defaults)
VIRIDIS = np.array([[0.267, 0.005, 0.329], [0.283, 0.141, 0.458], [0.254, 0.265, 0.530], [0.207, 0.372, 0.553],
                    [0.164, 0.471, 0.558], [0.128, 0.567, 0.551], [0.267, 0.679, 0.481], [0.993, 0.906, 0.144]], F)


# ------------------------------------------------------------------------------------------------ restatement ----
def restate_range(a, normalize, fixed=(-2.0, 2.0)):
    """computeRange, io_png.cpp:32-65."""
    if normalize == "fixed_range":
        return F(fixed[0]), F(fixed[1])
    v = a[np.isfinite(a)]
    n = int(v.size)
    if n == 0:
        return F(0.0), F(1.0)
    if normalize == "min_max":
        return v.min(), v.max()
    k1 = int(n * 0.01)                  # static_cast<size_t>(values.size() * 0.01): the same IEEE double product
    k99 = min(int(n * 0.99), n - 1)
    return np.partition(v, k1)[k1], np.partition(v, k99)[k99]


def _u8(x):
    assert x.dtype == F
    return x.astype(np.uint8)           # static_cast<uint8_t>: truncation (the values are in [0.5, 255.5])


def restate_image(a, start=(0, 0), normalize="percentile_1_99", colormap="viridis", align_to_world=True,
                  fixed=(-2.0, 2.0)):
    """(rgba uint8[rows, cols, 4], (vmin, vmax)) of layer `a` (rows x cols float32)."""
    a = np.asarray(a, dtype=F)
    rows, cols = a.shape
    vmin, vmax = restate_range(a, normalize, fixed)
    with np.errstate(all="ignore"):
        span = F(vmax - vmin)
        if span < F(1e-6):
            span = F(1.0)
        sr, sc = start if align_to_world else (0, 0)
        v = a[((np.arange(rows) + sr) % rows)[:, None], ((np.arange(cols) + sc) % cols)[None, :]]
        fin = np.isfinite(v)
        t = (v - vmin) / span
        t = np.where(t < F(1.0), t, F(1.0))   # std::min(1.0f, t)
        t = np.where(F(0.0) < t, t, F(0.0))   # std::max(0.0f, .)
        t = np.where(fin, t, F(0.0)).astype(F)
        assert t.dtype == F and span.dtype == F
        if colormap == "grayscale":
            g = _u8(t * F(255.0) + F(0.5))
            rgb = [g, g, g]
        elif colormap == "viridis":
            idx = t * F(7.0)
            i0 = idx.astype(np.int32)
            i1 = np.minimum(i0 + 1, 7)
            frac = idx - i0.astype(F)
            keep = F(1.0) - frac
            rgb = [_u8((VIRIDIS[i0, k] * keep + VIRIDIS[i1, k] * frac) * F(255.0) + F(0.5)) for k in range(3)]
        else:
            lo = np.zeros_like(t, dtype=np.uint8)
            hi = np.full_like(lo, 255)
            up1 = _u8(F(4.0) * t * F(255.0) + F(0.5))
            dn2 = _u8((F(1.0) - F(4.0) * (t - F(0.25))) * F(255.0) + F(0.5))
            up3 = _u8(F(4.0) * (t - F(0.5)) * F(255.0) + F(0.5))
            dn4 = _u8((F(1.0) - F(4.0) * (t - F(0.75))) * F(255.0) + F(0.5))
            q1, q2, q3 = t < F(0.25), t < F(0.5), t < F(0.75)
            rgb = [np.where(q2, lo, np.where(q3, up3, hi)),
                   np.where(q1, up1, np.where(q3, hi, dn4)),
                   np.where(q1, hi, np.where(q2, dn2, lo))]
    out = np.zeros((rows, cols, 4), dtype=np.uint8)
    for k in range(3):
        out[..., k] = np.where(fin, rgb[k], 0)
    out[..., 3] = np.where(fin, 255, 0)
    return out, (vmin, vmax)


def check(eng, a, start, **kw):
    """Render through the C ABI and hold pixels + range against the restatement of layer array `a`."""
    layer = kw.pop("layer")
    rgba, rng = eng.render_layer(layer, **kw)
    exp, erng = restate_image(a, start, **kw)
    assert rgba.shape == exp.shape and rgba.dtype == np.uint8
    bad = (rgba != exp).any(axis=2)
    assert not bad.any(), f"{layer} {kw}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0]}: " \
                          f"{rgba[bad][0]} vs {exp[bad][0]}; range {rng} vs {erng}"
    assert rng[0] == erng[0] and rng[1] == erng[1], (layer, kw, rng, erng)
    return rgba


def start_of(eng):
    g = eng.geometry()
    return g.start_row, g.start_col


# ----------------------------------------------------------------------------------------------------- the maps ----
ROWS, COLS, RES = 64, 48, 0.1   # 3 072 cells: one colour tile down, one (partial) across; 12 histogram blocks


def T(x=0.0, y=0.0, z=0.0):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def small_scan(seed, n=2500):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.4, 2.2, n).astype(F)   # (a strip of the map stays unobserved)
    y = rng.uniform(-2.6, 2.6, n).astype(F)
    z = (0.3 * np.sin(0.9 * x) * np.cos(0.7 * y) - 0.6 + 0.01 * rng.standard_normal(n)).astype(F)
    return {"x": x, "y": y, "z": z, "intensity": None, "rgb": None}


def special_layer(seed=5):
    """Everything the selection must order or keep out: NaN, both infinities, both signs, denormals, both zeros."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((ROWS, COLS)).astype(F)
    flat = a.reshape(-1)
    pick = rng.permutation(flat.size)
    flat[pick[:300]] = np.nan
    flat[pick[300:340]] = np.inf
    flat[pick[340:380]] = -np.inf
    flat[pick[380:420]] = F(1e-40)
    flat[pick[420:460]] = F(-3e-42)
    flat[pick[460:520]] = F(0.0)
    flat[pick[520:580]] = F(-0.0)
    flat[pick[580:600]] = np.finfo(F).max
    flat[pick[600:610]] = -np.finfo(F).max
    return a


N_SCANS = 9


def moved_pose(k):
    return T(0.37 * (k % 3), -0.23 * (k % 3))


def make_moved(gpu, est):
    cfg = gpu.capi.default_config()
    cfg.mode = 0
    cfg.estimation_type = 0 if est == "kalman" else 1
    eng = gpu.Engine(ROWS * RES, COLS * RES, RES, cfg)
    for k in range(N_SCANS):  # (the quantile estimator shows an elevation from a cell's fifth sample on)
        s = small_scan(k)
        rc, _ = eng.integrate(s["x"], s["y"], s["z"], T(z=0.6), moved_pose(k))
        assert rc == 0
    eng.add("user", 0.0)
    eng.set_layer("user", special_layer())
    return eng


@pytest.mark.parametrize("est", ["kalman", "p2"])
def test_every_setting_on_a_moved_map(gpu, est):
    """Record-backed `elevation`, an internal record field, and a user layer with its own array, after moves that leave the
    start index non-zero on both axes: every normalize x colormap x align_to_world combination."""
    eng = make_moved(gpu, est)
    start = start_of(eng)
    assert start[0] != 0 and start[1] != 0, start
    assert (eng.rows, eng.cols) == (ROWS, COLS)
    internal = "_kalman_p" if est == "kalman" else "_p2_q1"
    for layer in ("elevation", internal, "user"):
        a = eng.layer(layer)
        assert np.isfinite(a).sum() > 500 and (~np.isfinite(a)).sum() > 100, layer
        for normalize in NORMALIZE:
            for colormap in COLORMAP:
                img = {al: check(eng, a, start, layer=layer, normalize=normalize, colormap=colormap,
                                 align_to_world=al, fixed=FIXED) for al in (True, False)}
                assert not np.array_equal(img[True], img[False]), "align_to_world changes nothing on a moved map"
    # the defaults are the reference's: PERCENTILE_1_99, VIRIDIS, aligned, -2 .. 2
    d = gpu.capi.default_image_config()
    assert (d.normalize, d.colormap, d.align_to_world, d.fixed_min, d.fixed_max) == (1, 1, 1, -2.0, 2.0)
    rgba, rng = eng.render_layer("elevation")
    exp, erng = restate_image(eng.layer("elevation"), start)
    assert np.array_equal(rgba, exp) and rng == erng
    eng.close()


def finite_count_layer(n, seed):
    """Exactly n finite cells (distinct values of both signs), the rest NaN and infinities."""
    rng = np.random.default_rng(seed)
    flat = np.full(ROWS * COLS, np.nan, dtype=F)
    where = rng.permutation(flat.size)
    flat[where[n:]] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), flat.size - n)
    vals = np.unique(rng.standard_normal(2 * n + 8).astype(F))
    flat[where[:n]] = rng.permutation(vals)[:n]
    assert int(np.isfinite(flat).sum()) == n
    return flat.reshape(ROWS, COLS)


def tie_layer():
    """Runs of equal values that straddle rank int(n * 0.01) = 30 and rank int(n * 0.99) = 3041 of n = 3072."""
    s = np.sort(np.random.default_rng(11).standard_normal(ROWS * COLS).astype(F))
    s[22:41] = s[22]
    s[3035:3050] = s[3049]
    assert s[29] == s[30] == s[31] and s[3040] == s[3041] == s[3042]
    return np.random.default_rng(12).permutation(s).reshape(ROWS, COLS)


CASES = {
    "specials": special_layer,
    "all_equal": lambda: np.full((ROWS, COLS), F(0.731)),
    "all_equal_negative": lambda: np.full((ROWS, COLS), F(-5.5)),
    "signed_zeros": lambda: np.random.default_rng(2).choice(np.array([0.0, -0.0, np.nan], F), (ROWS, COLS)),
    "ties": tie_layer,
    "denormals": lambda: (np.random.default_rng(3).integers(-4000, 4000, (ROWS, COLS)) * 1e-44).astype(F),
    "huge": lambda: np.clip(np.random.default_rng(4).standard_normal((ROWS, COLS)) * 1e38, -3.3e38, 3.3e38).astype(F),
}
for _n in (0, 1, 2, 99, 100, 101, 199, 200, 3071, 3072):
    CASES[f"finite_{_n}"] = (lambda n=_n: finite_count_layer(n, 100 + n))


@pytest.fixture(scope="module")
def upload_map(gpu):
    cfg = gpu.capi.default_config()
    eng = gpu.Engine(ROWS * RES, COLS * RES, RES, cfg)
    eng.add("user", 0.0)
    eng.set_start_index(9, 17)
    yield eng
    eng.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_selection_on_uploaded_layers(upload_map, case):
    """Layers that put the radix select at risk, uploaded into a layer with its own array and into the record-backed
    elevation: both data-driven ranges, each with the colour map that shows the most of t."""
    a = np.asfortranarray(CASES[case]())
    eng = upload_map
    for layer in ("user", "elevation"):
        eng.set_layer(layer, a)
        assert np.array_equal(eng.layer(layer).view(np.uint32), a.view(np.uint32))
        for normalize, colormap in (("percentile_1_99", "viridis"), ("min_max", "jet"), ("percentile_1_99", "grayscale")):
            check(eng, a, (9, 17), layer=layer, normalize=normalize, colormap=colormap, align_to_world=True)
    if case.startswith("finite_"):
        n = int(case.split("_")[1])
        _, rng = eng.render_layer("user")
        v = np.sort(a[np.isfinite(a)])
        expect = (v[int(n * 0.01)], v[min(int(n * 0.99), n - 1)]) if n else (F(0.0), F(1.0))
        assert rng == expect, (rng, expect)


def test_large_map_many_blocks(gpu):
    """1200 x 1200: 361 colour tiles, 2 048 histogram blocks that each take several rounds, the global merge."""
    cfg = gpu.capi.default_config()
    cfg.mode = 1
    eng = gpu.Engine(120.0, 120.0, 0.1, cfg)
    assert (eng.rows, eng.cols) == (1200, 1200)
    rng = np.random.default_rng(8)
    a = (0.4 * rng.standard_normal((1200, 1200)) + 1.5).astype(F)
    a[rng.random((1200, 1200)) < 0.2] = np.nan
    a[:3, :5] = -7.0
    a = np.asfortranarray(a)
    eng.set_layer("elevation", a)
    eng.set_start_index(700, 333)
    check(eng, a, (700, 333), layer="elevation")
    eng.close()


def test_tiled_engine_renders_its_window(gpu):
    cfg = gpu.capi.default_config()
    cfg.mode = 1
    tile = (32, 64, 100, 70, 40, 70, 80, 60)   # stored 100 x 70 window of a 200 x 160 buffer
    eng = gpu.Engine(20.0, 16.0, 0.1, cfg, tile=tile)
    assert (eng.s_rows, eng.s_cols) == (100, 70)
    a = np.asfortranarray(np.random.default_rng(9).standard_normal((100, 70)).astype(F))
    a[10:20, 30:33] = np.nan
    eng.set_layer("elevation", a)
    for al in (True, False):
        rgba = check(eng, a, (0, 0), layer="elevation", normalize="min_max", colormap="jet", align_to_world=al)
        assert rgba.shape == (100, 70, 4)
    eng.close()


def test_device_variant_and_size_query(gpu):
    eng = make_moved(gpu, "kalman")
    host, rng = eng.render_layer("elevation", colormap="jet")
    d_ptr, w, h, drng = eng.render_layer_device("elevation", colormap="jet")
    assert (w, h) == (COLS, ROWS) and drng == rng and d_ptr
    eng.sync()
    back = np.empty((h, w, 4), dtype=np.uint8)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(d_ptr), back.nbytes, 2) == 0
    assert np.array_equal(back, host)
    # without the range the call only enqueues; the image is the same once the stream has drained
    d2, _, _, none = eng.render_layer_device("elevation", colormap="jet", want_range=False)
    assert none is None
    eng.sync()
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(d2), back.nbytes, 2) == 0
    assert np.array_equal(back, host)
    # NULL / too small a buffer: the size, and nothing written
    lib, cfg = gpu.capi.load(), gpu.capi.default_image_config()
    wv, hv = C.c_int32(0), C.c_int32(0)
    small = np.full(16, 7, dtype=np.uint8)
    assert lib.fdm_engine_render_layer(eng._h, b"elevation", C.byref(cfg), small.ctypes.data_as(C.c_void_p), 16,
                                       C.byref(wv), C.byref(hv), None) == 0
    assert (wv.value, hv.value) == (COLS, ROWS) and (small == 7).all()
    eng.close()


def test_errors_and_the_map_is_untouched(gpu):
    eng = make_moved(gpu, "p2")
    before = {n: eng.layer(n).copy() for n in eng.layers()}
    geo = eng.geometry()
    lib = gpu.capi.load()
    cfg = gpu.capi.default_image_config()
    buf = np.zeros((ROWS, COLS, 4), dtype=np.uint8)
    w, h = C.c_int32(0), C.c_int32(0)

    def call(layer, cfg_ref, data=buf):
        return lib.fdm_engine_render_layer(eng._h, layer, cfg_ref, None if data is None else data.ctypes.data_as(C.c_void_p),
                                           0 if data is None else data.nbytes, C.byref(w), C.byref(h), None)
    assert call(b"no_such_layer", C.byref(cfg)) == gpu.capi.FDM_ERR_NO_LAYER
    assert call(b"no_such_layer", C.byref(cfg), None) == gpu.capi.FDM_ERR_NO_LAYER
    assert b"no_such_layer" in lib.fdm_last_error()
    assert call(None, C.byref(cfg)) == gpu.capi.FDM_ERR_INVALID
    assert call(b"elevation", None) == gpu.capi.FDM_ERR_INVALID
    for field, bad in (("normalize", 3), ("normalize", -1), ("colormap", 3), ("colormap", -1)):
        c = gpu.capi.default_image_config()
        setattr(c, field, bad)
        assert call(b"elevation", C.byref(c)) == gpu.capi.FDM_ERR_INVALID, (field, bad)
    d = C.c_void_p()
    assert lib.fdm_engine_render_layer_device(eng._h, b"nope", C.byref(cfg), C.byref(d), None, None, None) == \
        gpu.capi.FDM_ERR_NO_LAYER
    assert lib.fdm_engine_render_layer_device(eng._h, b"elevation", C.byref(cfg), None, None, None, None) == \
        gpu.capi.FDM_ERR_INVALID
    with pytest.raises(gpu.EngineError):
        eng.render_layer("no_such_layer")
    assert not buf.any()
    for normalize in NORMALIZE:
        for name in ("elevation", "variance", "_p2_q0"):
            eng.render_layer(name, normalize=normalize)
    assert eng.layers() == list(before)
    for n, a in before.items():
        assert np.array_equal(eng.layer(n).view(np.uint32), a.view(np.uint32)), n
    assert same_geometry(eng.geometry(), geo)
    eng.close()


def test_render_between_two_scans_of_a_stream(gpu, R):
    """A scan enqueued on the device leaves its update held back; a render in between launches it first and shows that
    scan; the stream then goes on bit-identical to the oracle."""
    import torch

    def fill(c):
        c.mode = 0
    eng, ref = pair(gpu, R, ROWS * RES, COLS * RES, RES, fill)
    Tbs = T(z=0.6)
    run_both(eng, ref, small_scan(20), Tbs, T())
    s = small_scan(21)
    d = {k: torch.from_numpy(s[k]).cuda() for k in ("x", "y", "z")}
    eng.integrate_device(d["x"], d["y"], d["z"], Tbs, T(0.31, 0.22))
    rc, _ = ref.integrate(s["x"], s["y"], s["z"], Tbs, T(0.31, 0.22))
    assert rc == 0
    g = ref.geometry()
    rgba, rng = eng.render_layer("elevation", normalize="min_max", colormap="grayscale")
    exp, erng = restate_image(ref.layer("elevation"), (g.start_row, g.start_col), normalize="min_max",
                              colormap="grayscale")
    assert np.array_equal(rgba, exp) and rng == erng
    run_both(eng, ref, small_scan(22), Tbs, T(0.5, 0.5))
    assert_layers_bit_identical(eng, ref)
    assert same_geometry(eng.geometry(), ref.geometry())
    eng.close()
