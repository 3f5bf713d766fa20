"""Cases that reach every kernel the stencil stages choose between (fastdem_amd/csrc/fdm_engine_post.inl dispatches,
fastdem_amd/csrc/fdm_post.hpp holds the kernels), with the name of the kernel each case must run.  Test data:
tests/test_post_cases.py proves on the CPU that every case does what it is meant to (the oracle writes enough cells, a
`min_valid` case splits them, the adversarial field puts a tie, a signed zero, a dropped weight and an inverted pair
into one neighbourhood) and that the names expected here are exactly the launch sites of the source;
tests/test_post_dispatch_gpu.py holds the engine to the oracle on them, bit for bit, and to the expected name.

The thresholds are the repository's own formulas restated (each function names the one it restates); the constants they
use are compared with the source by tests/test_post_cases.py.  Plain NumPy: neither the engine nor the oracle.
"""
import collections
import functools

import numpy as np

F32 = np.float32

# ---- constants of fdm_post.hpp / fdm_engine_post.inl (checked against the source by tests/test_post_cases.py) --------
K_MAX_REGION = 256          # kMaxRegion
S3R, S3C = 32, 8            # kS3R_, kS3C_: the tile of k_median_sel / k_features_sel
FUSION_WAVE_MAX = 1024      # kFusionWaveMax
FUS_HALO_MAX = 8            # kFusHaloMax
FEAT_HALO_MAX = 16          # kFeatHaloMax
FEAT_TILE = (32, 16)        # kFeatTileR, kFeatTileC
LDS_CAP = 160 * 1024        # the `160u * 1024u` both selection kernels are held to
POOL_THREADS = 16384        # ensure_pool: threads in flight of a pooled kernel, each walks the map with that stride
MAX_LIST_MOVES = 1.0e9      # what a pooled case may cost here: entries^2 / 4 list moves per finite cell, over the map

RES = 0.02
# name: (width, height, rows, cols, the move that rolls the buffer seam across the map)
MAPS = {
    "small": (0.74, 0.42, 37, 21, (0.07, -0.05)),    # neither side a multiple of 4: every tile is a partial one
    "strip": (0.10, 1.40, 5, 70, (0.07, -0.05)),     # narrower than any kernel's tile
    "tall": (1.94, 0.46, 97, 23, (0.07, -0.05)),     # longer than the largest windows reach: they differ from cell to cell
    "grid": (2.60, 2.60, 130, 130, (0.07, -0.05)),   # 16 900 cells: 516 threads of a pooled kernel take a second cell
}


# ---- the formulas ----------------------------------------------------------------------------------------------------
def median_sel_lds_bytes(kernel):
    """median_sel_lds_bytes (fdm_post.hpp)."""
    h = kernel // 2
    return (S3R + 2 * h) * (S3C + 2 * h) * 4


def features_sel_lds_bytes(halo, n_entries):
    """features_sel_lds_bytes (fdm_post.hpp)."""
    return (S3R + 2 * halo) * (S3C + 2 * halo) * 8 + n_entries * 4


@functools.lru_cache(maxsize=None)
def region_disc(radius, res=RES):
    """region_disc (fdm_engine_post.inl), in its float arithmetic: (dr, dc) int arrays, dr-major / dc-minor."""
    radius, res = F32(radius), F32(res)
    k = int(np.floor(F32(F32(radius / res) + F32(1e-4))))
    r2 = F32(radius * radius)
    lim = F32(r2 * F32(F32(1.0) + F32(1e-5)))
    d = np.arange(-k, k + 1)
    dr, dc = (a.ravel() for a in np.meshgrid(d, d, indexing="ij"))
    d2 = (dr * dr + dc * dc).astype(F32) * F32(res * res)
    keep = d2 <= lim
    return dr[keep], dc[keep]


def reach(radius, res=RES):
    """`halo` of the dispatch: the farthest row / column offset of the disc."""
    dr, dc = region_disc(radius, res)
    return int(max(np.abs(dr).max(), np.abs(dc).max()))


def need_lo_hi(n_entries, lo_pct, hi_pct):
    """need_lo / need_hi (fdm_engine_apply_feature_extraction): the order statistics `step` can ask for, counted from the
    bottom and from the top of the full region."""
    lo_pct, hi_pct, top = F32(lo_pct), F32(hi_pct), F32(n_entries - 1)
    return int(F32(lo_pct * top)) + 1, (n_entries - 1) - int(F32(hi_pct * top)) + 1


def median_kernel(kernel):
    """The dispatch of fdm_engine_apply_spatial_smoothing."""
    side = 2 * (kernel // 2) + 1
    if kernel == 3:
        return "k_median3_tiled"
    if side * side <= K_MAX_REGION:
        return "k_median"
    return "k_median_sel" if median_sel_lds_bytes(kernel) <= LDS_CAP else "k_median_big"


def fusion_n_pad(n_entries):
    n_pad = 64
    while n_pad < n_entries:
        n_pad <<= 1
    return n_pad


def fusion_kernel(radius, q_lower, q_upper, res=RES):
    """The dispatch of fdm_engine_apply_uncertainty_fusion."""
    n, halo = region_disc(radius, res)[0].size, reach(radius, res)
    q_ok = all(F32(1e-6) <= F32(q) <= F32(1.0) for q in (q_lower, q_upper))
    if n <= 29 and halo <= FUS_HALO_MAX and q_ok:
        return "k_fusion_f64_tiled<%d, true>" % n if n in (29, 25, 21, 13, 9, 5) else "k_fusion_f64_tiled<29, false>"
    if n <= 32 and halo <= FUS_HALO_MAX:
        return "k_fusion_net32_tiled"
    return "k_fusion_wave" if n <= FUSION_WAVE_MAX else "k_fusion_big"


def features_kernel(radius, lo_pct, hi_pct, res=RES):
    """The dispatch of fdm_engine_apply_feature_extraction."""
    n, halo = region_disc(radius, res)[0].size, reach(radius, res)
    need_lo, need_hi = need_lo_hi(n, lo_pct, hi_pct)
    pct_ok = 0.0 <= F32(lo_pct) <= 1.0 and 0.0 <= F32(hi_pct) <= 1.0
    near = pct_ok and need_lo <= 16 and need_hi <= 16
    if near and halo <= FEAT_HALO_MAX and n <= K_MAX_REGION:
        for klo, khi, name in ((2, 3, "<2, 3>"), (4, 4, "<4, 4>"), (6, 7, "<6, 7>"), (8, 8, "<8>")):
            if need_lo <= klo and need_hi <= khi:
                return "k_features_tiled" + name
        return "k_features_tiled<16>"
    if near:
        return "k_features<8>" if need_lo <= 8 and need_hi <= 8 else "k_features<16>"
    return "k_features_sel" if features_sel_lds_bytes(halo, n) <= LDS_CAP else "k_features_big"


def cells(c):
    """A radius of c cells, in metres."""
    return c * RES


# ---- fields ----------------------------------------------------------------------------------------------------------
def terrain(rng, shape, holes=0.3, noise=0.02):
    r, c = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    z = 0.4 * np.sin(r * 0.11) * np.cos(c * 0.07) + 0.002 * r + rng.normal(0, noise, shape)
    z = z.astype(F32)
    z[rng.uniform(size=shape) < holes] = np.nan
    return z


def bound_field(shape, seed, holes=0.35):
    """(upper_bound, lower_bound) built to trip a fusion kernel: a plateau of equal bounds (ties keep the entry order),
    -0.0 / +0.0, pairs so far apart that the weight is <= 1e-6 (counted as valid, never sampled), inverted pairs (a
    negative range: a negative or huge weight) and holes."""
    rng = np.random.default_rng(seed)
    el = terrain(rng, shape, holes=holes)
    half = np.abs(rng.normal(0.05, 0.03, shape)).astype(F32) + F32(0.005)
    up, lo = el + half, el - half
    box = (slice(shape[0] // 12, shape[0] // 4), slice(shape[1] // 12, shape[1] // 4))
    up[box] = np.where(np.isfinite(up[box]), F32(0.25), up[box])
    lo[box] = np.where(np.isfinite(lo[box]), F32(-0.125), lo[box])
    z = rng.uniform(size=shape) < 0.05
    lo[z & np.isfinite(lo)] = F32(-0.0)
    z2 = rng.uniform(size=shape) < 0.05
    up[z2 & np.isfinite(up) & (lo <= 0)] = F32(0.0)
    far = rng.uniform(size=shape) < 0.05
    up[far & np.isfinite(up)] = F32(3.0e6)
    inv = rng.uniform(size=shape) < 0.02
    up[inv & np.isfinite(up)] = F32(-5.0)
    return up, lo


def plant_traps(up, lo):
    """All of the above within one cell of the map's centre, so that the smallest disc tested holds every one of them at
    once (by chance that takes a disc of ~100 cells): a tie in both bounds, a tie in the lower bound alone, -0.0 and +0.0
    as lower bounds, a weight <= 1e-6 and an inverted pair."""
    r, c = up.shape[0] // 2, up.shape[1] // 2
    pairs = ((0.25, -0.125), (0.25, -0.125), (0.5, -0.125), (0.0625, -0.0), (0.03125, 0.0), (3.0e6, -0.25), (-5.0, 0.125),
             (0.0, -0.0625), (-0.0, -0.03125))
    for k, (u, l) in enumerate(pairs):
        up[r - 1 + k // 3, c - 1 + k % 3], lo[r - 1 + k // 3, c - 1 + k % 3] = F32(u), F32(l)


def elevation_field(shape, seed, holes=0.25):
    """Terrain for the median and the feature stages: spikes, plateaus of equal heights (ties among the order
    statistics), exact zeros and holes.  No -0.0: std::nth_element leaves the order of -0.0 and +0.0 unspecified."""
    rng = np.random.default_rng(seed)
    el = terrain(rng, shape, holes=0.0, noise=0.01)
    el[rng.uniform(size=shape) < 0.03] = F32(50.0)
    el[rng.uniform(size=shape) < 0.02] = F32(-7.5)
    flat = rng.uniform(size=shape) < 0.15
    el[flat] = np.round(el[flat] * F32(8.0)) / F32(8.0)
    el[rng.uniform(size=shape) < 0.03] = F32(0.0)
    el[rng.uniform(size=shape) < holes] = np.nan
    el[el == 0] = F32(0.0)
    return el


def sparse_elevation_field(shape, seed, finite=0.03):
    """The same with only `finite` of the cells holding a height, for the pooled feature kernel on the large map.  Cell
    pairs POOL_THREADS apart in the kernels' cell order (column-major) are planted: one thread, two finite cells."""
    rng = np.random.default_rng(seed)
    el = elevation_field(shape, seed + 1, holes=0.0)
    el[rng.uniform(size=shape) >= finite] = np.nan
    full = elevation_field(shape, seed + 1, holes=0.0)
    for t in stride_pairs(shape):
        for u in (t, t + POOL_THREADS):
            el[u % shape[0], u // shape[0]] = full[u % shape[0], u // shape[0]]
    return el


def stride_pairs(shape):
    """First cells t (cell order of the pooled kernels: t = column * rows + row) whose thread also owns t + POOL_THREADS."""
    spare = shape[0] * shape[1] - POOL_THREADS
    return [t for t in (0, 1, 77, 255, 256, 400, spare - 1) if 0 <= t < spare]


@functools.lru_cache(maxsize=None)
def field(name, map_name):
    """The layers of a case, read-only: {"elevation": ...} or {"upper_bound": ..., "lower_bound": ...}."""
    shape = MAPS[map_name][2:4]
    seed = {"small": 101, "strip": 103, "grid": 107, "tall": 109}[map_name]
    if name == "bounds":
        up, lo = bound_field(shape, seed)
        plant_traps(up, lo)
        out = {"upper_bound": up, "lower_bound": lo}
    elif name == "bounds_thin":       # half the cells empty: k_fusion_big on the large map stays under MAX_LIST_MOVES
        up, lo = bound_field(shape, seed, holes=0.5)
        plant_traps(up, lo)
        out = {"upper_bound": up, "lower_bound": lo}
    elif name == "elevation":
        out = {"elevation": elevation_field(shape, seed)}
    elif name == "elevation_thin":    # 40 % of the cells empty: the pooled kernels on the tall map stay under MAX_LIST_MOVES
        out = {"elevation": elevation_field(shape, seed, holes=0.4)}
    elif name == "elevation_sparse":
        out = {"elevation": sparse_elevation_field(shape, seed)}
    else:
        raise KeyError(name)
    for a in out.values():
        a.setflags(write=False)
    return out


def neighbour_counts(ok, radius):
    """Per cell: how many cells of the disc lie inside the map and are set in `ok` (the centre included)."""
    dr, dc = region_disc(radius)
    rows, cols = ok.shape
    k = max(int(np.abs(dr).max()), int(np.abs(dc).max()))
    pad = np.zeros((rows + 2 * k, cols + 2 * k), dtype=np.int32)
    pad[k:k + rows, k:k + cols] = ok
    out = np.zeros(ok.shape, dtype=np.int32)
    for a, b in zip(dr, dc):
        out += pad[k + a:k + a + rows, k + b:k + b + cols]
    return out


def split_min_valid(field_name, map_name, radius):
    """The `min_valid` that admits about half of the cells with a finite centre: the median of their neighbour counts."""
    lay = field(field_name, map_name)
    ok = np.ones(MAPS[map_name][2:4], dtype=bool)
    for a in lay.values():
        ok &= np.isfinite(a)
    return int(np.median(neighbour_counts(ok, radius)[ok]))


def list_moves(case):
    """What a pooled case costs: (finite entries)^2 / 4 list moves per finite cell, the finite entries of a cell taken as
    the disc's (or the box's, or the map's if that is smaller) times the finite share of the field."""
    lay = field(case.field, case.map)
    ok = np.ones(MAPS[case.map][2:4], dtype=bool)
    for a in lay.values():
        ok &= np.isfinite(a)
    if case.stage == "median":
        entries = (2 * (case.params[0] // 2) + 1) ** 2
    else:
        entries = region_disc(case.params[0])[0].size
    entries = min(entries, ok.size) * ok.mean()
    return entries * entries / 4.0 * ok.sum()


# ---- the cases -------------------------------------------------------------------------------------------------------
# stage: "inpaint" (iterations, min_valid, inplace) | "median" (kernel_size, min_valid) |
#        "fusion" (radius, sigma, q_lower, q_upper, min_valid) | "features" (radius, min_valid, lo_pct, hi_pct)
# kernel: what Engine.debug_last_post_kernel() must say after the call; again: the parameters of the third call of the
# case (a changed radius / size: another region table, another pool), split: `min_valid` was chosen to split the cells.
Case = collections.namedtuple("Case", "id stage map field params kernel again split")
FEATURE_LAYERS = ("step", "slope", "roughness", "curvature", "_normal_x", "_normal_y", "_normal_z")
OUTPUTS = {"inpaint": ("elevation", "elevation_inpainted"), "median": ("elevation",),
           "fusion": ("upper_bound", "lower_bound"), "features": FEATURE_LAYERS}

MEDIAN_SEL_MAX = max(k for k in range(17, 400) if median_sel_lds_bytes(k) <= LDS_CAP)        # 183: 162 640 B
FEATURES_SEL_REACH = max(h for h in range(10, 80)
                         if features_sel_lds_bytes(h, region_disc(cells(h))[0].size) <= LDS_CAP)  # 53 cells
# the radius of that reach with the most entries the LDS still takes, and the first radius of the next reach
FEATURES_SEL_RADIUS = max(FEATURES_SEL_REACH + j / 10.0 for j in range(10)
                          if features_sel_lds_bytes(FEATURES_SEL_REACH, region_disc(cells(FEATURES_SEL_REACH + j / 10.0))[0].size)
                          <= LDS_CAP)
FEATURES_BIG_RADIUS = FEATURES_SEL_REACH + 1.0

# fusion discs on the 0.02 m map: radius in cells -> (cells of the disc, n_pad of k_fusion_wave or None for k_fusion_big)
FUSION_DISCS = {3.2: (37, 64), 4.5: (69, 128), 6.5: (137, 256), 9.1: (261, 512), 18.0: (1009, 1024), 18.1: (1033, None)}
FUSION_AGAIN = {3.2: 3.7, 4.5: 5.0, 6.5: 6.1, 9.1: 8.3, 18.0: 17.5, 18.1: 18.5}
QUANTILES = ((0.01, 0.99), (1e-6, 1.0), (0.0, 1.0), (0.5, 0.5))


def _cases():
    out = []

    def add(id_, stage, map_, fld, params, kernel, again, split=False):
        out.append(Case(id_, stage, map_, fld, tuple(params), kernel, tuple(again), split))

    for m in ("small", "strip"):
        add(f"inpaint-{m}", "inpaint", m, "elevation", (3, 2, False), "k_inpaint_pass_tiled", (2, 1, True))
    add("inpaint-none", "inpaint", "small", "elevation", (0, 2, False), "", (1, 3, False))
    # ---- median: box of 2 * (k / 2) + 1 cells a side
    add("median-3", "median", "small", "elevation", (3, 5), "k_median3_tiled", (5, 5))
    add("median-14", "median", "small", "elevation", (14, 5), "k_median", (12, 9))          # even: the 15-wide box, 225 cells
    add("median-15", "median", "small", "elevation", (15, 30), "k_median", (13, 1))         # the largest box of <= 256 cells
    add("median-16", "median", "small", "elevation", (16, 5), "k_median_sel", (18, 9))      # even: the 17-wide box, 289 cells
    add("median-17", "median", "small", "elevation", (17, 40), "k_median_sel", (19, 1))     # k_median_sel at its smallest
    for m in ("small", "strip"):
        k = MEDIAN_SEL_MAX
        add(f"median-{k}-{m}", "median", m, "elevation", (k, 5), "k_median_sel", (k - 2, 9))       # the largest LDS granted
        add(f"median-{k + 1}-{m}", "median", m, "elevation", (k + 1, 5), "k_median_big", (k + 3, 9))
    # (on the small map and the strip such a window is the whole map; on the tall one it is cut off at a different row
    #  for the cells of the first and the last rows)
    add(f"median-{k}-tall", "median", "tall", "elevation_thin", (k, 5), "k_median_sel", (k - 20, 9))
    add(f"median-{k + 1}-tall", "median", "tall", "elevation_thin", (k + 1, 5), "k_median_big", (k + 21, 9))
    # ---- fusion on the adversarial field: every n_pad of k_fusion_wave, then k_fusion_big
    for c, (n, n_pad) in FUSION_DISCS.items():
        kern = "k_fusion_wave" if n_pad else "k_fusion_big"
        tag = f"wave{n_pad}" if n_pad else "big"
        for ql, qu in QUANTILES:
            add(f"fusion-{tag}-q{ql:g}-{qu:g}", "fusion", "small", "bounds", (cells(c), 0.1, ql, qu, 1), kern,
                (cells(FUSION_AGAIN[c]), 0.1, ql, qu, 3))
        mv = split_min_valid("bounds", "small", cells(c))
        add(f"fusion-{tag}-split", "fusion", "small", "bounds", (cells(c), 0.05, 0.01, 0.99, mv), kern,
            (cells(FUSION_AGAIN[c]), 0.05, 0.25, 0.75, mv), split=True)
    add("fusion-wave256-strip", "fusion", "strip", "bounds", (cells(6.5), 0.1, 0.01, 0.99, 3), "k_fusion_wave",
        (cells(6.1), 0.1, 0.01, 0.99, 3))
    add("fusion-big-strip", "fusion", "strip", "bounds", (cells(18.1), 0.1, 0.01, 0.99, 3), "k_fusion_big",
        (cells(18.5), 0.1, 0.01, 0.99, 3))
    add("fusion-big-grid", "fusion", "grid", "bounds_thin", (cells(18.1), 0.1, 0.01, 0.99, 5), "k_fusion_big",
        (cells(18.5), 0.1, 0.05, 0.95, 5))
    # ---- feature extraction (all seven layers; correctly rounded trig on the oracle's side)
    for c in (7, 8, 9):   # 149, 197, 253 entries: the defaults ask for 8 / 9, 10 / 11, 13 / 14 order statistics
        add(f"features-tiled-reach{c}", "features", "small", "elevation", (cells(c), 4, 0.05, 0.95), "k_features_tiled<16>",
            (cells(c - 0.5), 4, 0.05, 0.95))
    mv = split_min_valid("elevation", "small", cells(8))
    add("features-tiled-split", "features", "small", "elevation", (cells(8), mv, 0.0, 1.0), "k_features_tiled<2, 3>",
        (cells(7.5), mv, 0.0, 1.0), split=True)
    add("features-tiled-reach9-strip", "features", "strip", "elevation", (cells(9), 4, 0.05, 0.95), "k_features_tiled<16>",
        (cells(8.5), 4, 0.05, 0.95))
    add("features-top8", "features", "small", "elevation", (cells(15), 4, 0.0, 1.0), "k_features<8>",       # 709 cells
        (cells(14.5), 4, 0.0, 1.0))
    add("features-top16", "features", "small", "elevation", (cells(15), 4, 0.015, 0.985), "k_features<16>",  # 11 / 12
        (cells(14.5), 4, 0.015, 0.985))
    add("features-top16-strip", "features", "strip", "elevation", (cells(15), 4, 0.015, 0.985), "k_features<16>",
        (cells(14.5), 4, 0.015, 0.985))
    for m in ("small", "strip"):
        add(f"features-sel-max-{m}", "features", m, "elevation", (cells(FEATURES_SEL_RADIUS), 4, 0.05, 0.95), "k_features_sel",
            (cells(FEATURES_SEL_REACH - 3.5), 4, 0.3, 0.7))
        add(f"features-big-{m}", "features", m, "elevation", (cells(FEATURES_BIG_RADIUS), 4, 0.05, 0.95), "k_features_big",
            (cells(FEATURES_BIG_RADIUS + 2.5), 4, 0.3, 0.7))
    add("features-sel-max-tall", "features", "tall", "elevation_thin", (cells(FEATURES_SEL_RADIUS), 4, 0.05, 0.95),
        "k_features_sel", (cells(FEATURES_SEL_REACH - 3.5), 4, 0.3, 0.7))
    add("features-big-tall", "features", "tall", "elevation_thin", (cells(FEATURES_BIG_RADIUS), 4, 0.05, 0.95),
        "k_features_big", (cells(FEATURES_BIG_RADIUS + 2.5), 4, 0.3, 0.7))
    add("features-big-grid", "features", "grid", "elevation_sparse", (cells(FEATURES_BIG_RADIUS), 4, 0.05, 0.95),
        "k_features_big", (cells(FEATURES_BIG_RADIUS + 2.5), 4, 0.3, 0.7))
    return out


CASES = _cases()
POOLED = ("k_median_big", "k_fusion_big", "k_features_big")


def kernel_of(stage, params):
    """The name the restated dispatch gives a call."""
    if stage == "inpaint":
        return "k_inpaint_pass_tiled" if params[0] > 0 else ""
    if stage == "median":
        return median_kernel(params[0])
    if stage == "fusion":
        return fusion_kernel(params[0], params[2], params[3])
    return features_kernel(params[0], params[2], params[3])


def set_layers(obj, case):
    for name, a in field(case.field, case.map).items():
        obj.set_layer(name, a)


def apply(obj, stage, params):
    """The same call on an engine or on the oracle."""
    if stage == "inpaint":
        obj.apply_inpainting(*params)
    elif stage == "median":
        obj.apply_spatial_smoothing("elevation", *params)
    elif stage == "fusion":
        obj.apply_uncertainty_fusion(True, *params)
    else:
        obj.apply_feature_extraction(*params)
