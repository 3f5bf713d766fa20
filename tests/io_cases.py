"""The inputs of the I/O edge tests, built once and shared: tests/test_io_restate_vs_oracle.py runs every one of them
through the oracle and the NumPy restatement on the CPU, tests/test_egress_edges_gpu.py and
tests/test_ingest_edges_gpu.py run the same ones through the HIP engine.  Test data, not product.

Egress (fdm_egress.hpp): count per 256-thread block -> one-block scan carrying across 1024-entry chunks -> ranked
write.  The cases sit on the partial last block, on blocks that keep nothing / everything, on the chunk carry, on the
rank of lane 63 and of wave 3, and on the record widths around the 64 KB LDS line of the write kernel.
Ingest (fdm_ingest.hpp): the same scheme over the points of a message."""
import numpy as np

from cloud2 import Layout, make_blob

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)


# ======================================================================================================= egress ====
class MapCase:
    """One map and the packs taken of it.  `layers`: [(name, float32[rows, cols] by buffer index)], created in this
    order when missing.  `fields`: user layers u00, u01, ... are added until a record has that many fields."""

    def __init__(self, name, rows, cols, res=0.5, start=(0, 0), position=(0.0, 0.0), move=None, est=0,
                 elevation=None, layers=(), fields=None, color=False, fill_defaults=False,
                 elevation_layer="elevation", subs=(None,), options=None, seed=0):
        self.name, self.rows, self.cols, self.res = name, rows, cols, res
        self.start, self.position, self.move, self.est = start, position, move, est
        self.elevation, self.layers, self.fields, self.color = elevation, list(layers), fields, color
        self.fill_defaults, self.elevation_layer, self.subs = fill_defaults, elevation_layer, list(subs)
        self.options, self.seed = options or {}, seed

    def __repr__(self):
        return self.name

    def fill_cfg(self, cfg):
        cfg.estimation_type = self.est
        return cfg

    def create(self, make):
        """make(width, height, resolution, fill_cfg, position) -> an Engine or a RefEngine, then filled."""
        obj = make(self.rows * self.res, self.cols * self.res, self.res, self.fill_cfg, self.position)
        assert (obj.rows, obj.cols) == (self.rows, self.cols), (obj.rows, obj.cols)
        for k, v in self.options.items():
            obj.set_option(k, v)       # (engine-only cases)
        if self.move:
            obj.move(*self.move)       # clears the strips it exposes: the layers are written afterwards
        rng = np.random.default_rng(1000 + self.seed)
        written = {}

        def put(name, arr):
            if not obj.exists(name):
                obj.add(name)
            written[name] = np.asfortranarray(arr, dtype=F32)
            obj.set_layer(name, written[name])

        put("elevation", self.elevation if self.elevation is not None else holes(rng, self.rows, self.cols, 0.3))
        if self.fill_defaults:         # every estimator layer its own values: a wrong stride or offset shows
            for name in obj.layers():
                if name != "elevation" and not name.startswith("_"):
                    put(name, wild(rng, self.rows, self.cols))
        for name, arr in self.layers:
            put(name, arr)
        if self.color:
            put("color", rng.integers(0, 1 << 24, (self.rows, self.cols), dtype=np.uint32).view(F32))
        if self.fields is not None:
            k = 0
            while record_fields(obj.layers(), self.elevation_layer) < self.fields:
                put("u%02d" % k, wild(rng, self.rows, self.cols))
                k += 1
            assert record_fields(obj.layers(), self.elevation_layer) == self.fields
        if self.start != (0, 0):
            obj.set_start_index(*self.start)
        g = obj.geometry()
        if not self.move:
            assert (g.start_row, g.start_col) == tuple(self.start)
        return obj, written


def record_fields(names, elevation_layer):
    """Width of a record of a map with these layers (x, y, z + float layers + rgb)."""
    return 3 + sum(1 for n in names if not n.startswith("_") and n != elevation_layer and n != "color") + \
        ("color" in names)


def holes(rng, rows, cols, p):
    a = rng.normal(0.0, 1.0, (rows, cols)).astype(F32)
    a[rng.random((rows, cols)) < p] = np.nan
    return a


def wild(rng, rows, cols):
    """Layer values that are copied as bits and gate nothing: NaN and both infinities among them."""
    a = rng.normal(0.0, 3.0, (rows, cols)).astype(F32)
    u = rng.random((rows, cols))
    a[u < 0.10] = np.nan
    a[(u >= 0.10) & (u < 0.15)] = np.inf
    a[(u >= 0.15) & (u < 0.20)] = -np.inf
    return a


def by_visit(values, rows, cols, start):
    """float32[rows, cols] by buffer index whose cells, in the full-map visiting order (column by column from the
    start index), hold `values`."""
    t = np.arange(rows * cols)
    r, c = (start[0] + t % rows) % rows, (start[1] + t // rows) % cols
    a = np.empty((rows, cols), dtype=F32)
    a[r, c] = np.asarray(values, dtype=F32)
    return a


def _patterns(tag, rows, cols, start):
    n = rows * cols
    t = np.arange(n)
    base = (0.25 * t - 7.0).astype(F32)

    def only(k):
        v = np.full(n, np.nan, F32)
        v[k] = base[k]
        return v

    special = np.array([np.inf, -np.inf, -0.0, 1e-45, FLT_MAX, -FLT_MAX, 1.5, np.nan, 0.0, -1e-39], dtype=F32)
    pats = {
        "all_valid": base,
        "none_valid": np.full(n, np.nan, F32),
        "only_first_lane": only(0),
        "only_lane63_of_wave3": only(255),
        "only_last_cell": only(n - 1),
        "waves_1_and_3": np.where(((t % 256) // 64) % 2 == 1, base, F32(np.nan)).astype(F32),
        "special_values": special[t % special.size],
    }
    return [MapCase(f"{tag}_{k}", rows, cols, start=start, elevation=by_visit(v, rows, cols, start), seed=i)
            for i, (k, v) in enumerate(pats.items())]


def _user(seed, rows, cols):
    return wild(np.random.default_rng(seed), rows, cols)


SUBMAPS_24x18 = [(5, 7, 0, 4), (5, 7, 4, 0), (23, 17, 1, 1), (6, 0, 1, 18), (0, 11, 24, 1), (23, 17, 24, 18)]
BAD_SUBMAPS_24x18 = [(24, 0, 1, 1), (0, 0, 25, 1), (3, 3, 2, -1), (-1, 0, 1, 1)]

EGRESS_CASES = (
    # ---- record widths on a two-block map (260 cells, the second block partial) ----
    [MapCase("fields_natural", 20, 13, start=(3, 5), seed=1)] +
    [MapCase(f"fields_{f}", 20, 13, start=(3, 5), fields=f, seed=f) for f in (63, 64, 65, 67)] +
    [MapCase("fields_68_with_colour", 20, 13, start=(3, 5), fields=68, color=True, seed=68)] +
    # ---- cell counts around one block ----
    [MapCase("cells_1", 1, 1, elevation=np.array([[2.5]], F32), seed=2),
     MapCase("cells_255", 15, 17, start=(7, 11), seed=3),
     MapCase("cells_256", 16, 16, start=(5, 9), seed=4),
     MapCase("cells_257_row", 1, 257, start=(0, 130), seed=5),
     MapCase("cells_257_col", 257, 1, start=(130, 0), seed=6)] +
    # ---- the scan's 1024-entry chunk (262 144 cells) ----
    [MapCase("scan_1024_blocks_less_a_cell", 511, 513, res=0.05, start=(100, 400), seed=7,
             elevation=holes(np.random.default_rng(70), 511, 513, 0.4)),
     MapCase("scan_1024_blocks", 512, 512, res=0.05, start=(511, 1), seed=8,
             elevation=holes(np.random.default_rng(71), 512, 512, 0.4)),
     MapCase("scan_1026_blocks", 513, 512, res=0.05, start=(17, 300), seed=9,
             elevation=holes(np.random.default_rng(72), 513, 512, 0.4))] +
    # ---- validity patterns ----
    _patterns("p16x16", 16, 16, (5, 9)) + _patterns("p20x13", 20, 13, (3, 5)) +
    # ---- submaps of a moved map ----
    [MapCase("submaps_moved", 24, 18, move=(3.6, -2.1), subs=[None] + SUBMAPS_24x18, seed=10,
             elevation=holes(np.random.default_rng(73), 24, 18, 0.2))] +
    # ---- storage and layer variants ----
    [MapCase("kalman_records", 20, 13, est=0, start=(3, 5), fill_defaults=True, seed=11, subs=[None, (18, 11, 7, 6)]),
     MapCase("p2_records", 20, 13, est=1, start=(3, 5), fill_defaults=True, seed=12, subs=[None, (18, 11, 7, 6)]),
     MapCase("elevation_is_user_layer", 20, 13, start=(3, 5), seed=13, elevation_layer="u00",
             layers=[("u00", holes(np.random.default_rng(74), 20, 13, 0.5)), ("u01", _user(75, 20, 13))]),
     MapCase("elevation_is_elevation_min", 20, 13, start=(3, 5), seed=14, elevation_layer="elevation_min",
             layers=[("elevation_min", holes(np.random.default_rng(76), 20, 13, 0.5))]),
     MapCase("far_from_origin", 24, 18, res=0.05, position=(1.0e6 + 0.3, -2.5e5), start=(7, 4), seed=15,
             subs=[None, (20, 15, 9, 8)])]
)
# engine-only storage variant: one array per layer instead of cell records (option `records`)
EGRESS_ENGINE_ONLY = [
    MapCase("kalman_per_layer", 20, 13, est=0, start=(3, 5), fill_defaults=True, seed=11, options={"records": 0},
            subs=[None, (18, 11, 7, 6)]),
    MapCase("p2_per_layer", 20, 13, est=1, start=(3, 5), fill_defaults=True, seed=12, options={"records": 0},
            subs=[None, (18, 11, 7, 6)]),
]
EGRESS_TOO_WIDE = MapCase("fields_68_without_colour", 20, 13, start=(3, 5), fields=68, seed=69)   # 65 float layers


# ======================================================================================================= ingest ====
def xyz(rng, n, bad=0.08):
    """Points inside a 14 m square; `bad` of them with one non-finite coordinate (NaN, +Inf or -Inf)."""
    x, y = (rng.uniform(-7.0, 7.0, n).astype(F32) for _ in range(2))
    z = rng.normal(0.0, 0.3, n).astype(F32)
    hit = np.flatnonzero(rng.random(n) < bad)
    which = rng.integers(0, 3, hit.size)
    value = np.array([np.nan, np.inf, -np.inf], F32)[rng.integers(0, 3, hit.size)]
    for k, ch in enumerate((x, y, z)):
        ch[hit[which == k]] = value[which == k]
    return x, y, z


def _count_case(n):
    rng = np.random.default_rng(n)
    x, y, z = xyz(rng, n)
    if n > 1000:
        return make_blob(x, y, z, point_step=12, rng=rng) + (n, 0)
    idx = np.arange(n)
    return make_blob(x, y, z, intensity=idx.astype(F32), rgb=(idx * 2654435761) & 0xFFFFFFFF, point_step=20,
                     rng=rng) + (n, 0)


def _density_case(kind):
    n = 512
    rng = np.random.default_rng(512)
    x, y, z = xyz(rng, n, bad=0.0)
    i = np.arange(n)
    nan, inf = F32(np.nan), F32(np.inf)
    if kind == "none_finite":
        x[:], y[::2], z[::3] = nan, inf, -inf
    elif kind in ("only_255", "only_511"):
        keep = 255 if kind == "only_255" else 511
        x[i != keep] = nan
    elif kind == "alternate_waves":
        z[(i // 64) % 2 == 0] = -inf
    elif kind in ("x_only", "y_only", "z_only"):
        ch = {"x_only": x, "y_only": y, "z_only": z}[kind]
        hit = rng.random(n) < 0.3
        ch[hit] = np.where(rng.random(int(hit.sum())) < 0.5, nan, inf)
    else:
        assert kind == "all_finite"
    return make_blob(x, y, z, intensity=i.astype(F32), rgb=i * 65793, point_step=24, rng=rng) + (n, 0)


# FLOAT64 intensities and what static_cast<float> makes of them (one round-to-nearest-even)
F64_VALUES = np.array([
    1e300, -1e300,                                    # -> +-Inf
    1e-320, 1e-46, -1e-46,                            # -> +-0
    1e-40, -3e-42, 2.0 ** -149, 1.1754942e-38,        # the float32 denormal range
    2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -20), 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149,   # ties and near-ties down there
    np.nan, 0.0, -0.0,
    1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24,               # exactly halfway: to even, down and up
    -(1 + 2.0 ** -24), 1 + 2.0 ** -24 + 2.0 ** -50,   # just above halfway: up
    FLT_MAX * (1 + 2.0 ** -25),                       # below the halfway point to 2^128: FLT_MAX
    FLT_MAX * (1 + 2.0 ** -24), -FLT_MAX * (1 + 2.0 ** -24),   # past it: Inf
    FLT_MAX, 0.1, 123456.789, -2.5,
], dtype=np.float64)


def _f64_case(off, step):
    n = 4 * F64_VALUES.size + 3
    rng = np.random.default_rng(off)
    x, y, z = xyz(rng, n, bad=0.1)
    return make_blob(x, y, z, intensity=F64_VALUES[np.arange(n) % F64_VALUES.size], intensity_type=8,
                     offsets=dict(intensity=off), point_step=step, rng=rng) + (n, 0)


def _type_case(itype):
    n = 300
    rng = np.random.default_rng(40 + itype)
    x, y, z = xyz(rng, n)
    blob, lay = make_blob(x, y, z, intensity=rng.integers(1, 250, n), intensity_type=5, point_step=16, rng=rng)
    lay.intensity_type = itype     # the same non-zero bytes read as INT8 / INT16 / INT32 / UINT32 / an unknown code
    return blob, lay, n, 0


def _u16_case():
    n = 260
    rng = np.random.default_rng(46)
    x, y, z = xyz(rng, n)
    a = np.array([0, 255, 256, 65535])[np.arange(n) % 4]
    return make_blob(x, y, z, intensity=a, intensity_type=4, offsets=dict(intensity=13), point_step=15, rng=rng) + (n, 0)


def _layout_case(kind):
    n = 300
    rng = np.random.default_rng(47)
    x, y, z = xyz(rng, n)
    idx = np.arange(n)
    if kind == "ends_at_last_byte_f32":      # rgb's last byte is the record's last byte
        return make_blob(x, y, z, intensity=rng.random(n), rgb=idx * 65793, point_step=20, rng=rng) + (n, 0)
    if kind == "ends_at_last_byte_f64":      # the FLOAT64 intensity's
        return make_blob(x, y, z, intensity=rng.random(n), intensity_type=8, rgb=idx * 65793,
                         offsets=dict(rgb=12, intensity=16), point_step=24, rng=rng) + (n, 0)
    if kind == "ends_at_last_byte_u8":       # odd point_step, the UINT8 intensity on its last byte
        return make_blob(x, y, z, intensity=idx % 256, intensity_type=2, offsets=dict(intensity=12),
                         point_step=13, rng=rng) + (n, 0)
    if kind == "step_1024_far_end":
        return make_blob(x, y, z, intensity=idx % 60000, intensity_type=4, rgb=idx * 65793,
                         offsets=dict(intensity=1006, x=1008, y=1012, z=1016, rgb=1020), point_step=1024,
                         rng=rng) + (n, 0)
    lead = int(kind[-1])                     # an aligned layout in a blob that starts off a 4-byte boundary
    return make_blob(x, y, z, intensity=rng.random(n), intensity_type=8, rgb=idx * 65793,
                     offsets=dict(rgb=12, intensity=16), point_step=24, rng=rng, lead=lead) + (n, lead)


POINT_COUNTS = (1, 63, 64, 65, 255, 256, 257, 262_143, 262_144, 262_145, 262_401)
N_INTEGRATE = 262_145     # this blob also goes through integrate_cloud2: n_input summed over 1025 blocks
DENSITIES = ("all_finite", "none_finite", "only_255", "only_511", "alternate_waves", "x_only", "y_only", "z_only")
ZERO_TYPES = (1, 3, 5, 6, 9, 255, 0, -1)

# name -> builder of (blob, layout, n, lead)
INGEST_CASES = {}
INGEST_CASES.update({f"n_{n}": (lambda n=n: _count_case(n)) for n in POINT_COUNTS})
INGEST_CASES.update({f"density_{k}": (lambda k=k: _density_case(k)) for k in DENSITIES})
INGEST_CASES.update({f"f64_off{o}_step{s}": (lambda o=o, s=s: _f64_case(o, s))
                     for o, s in ((16, 24), (12, 20), (13, 23))})
INGEST_CASES.update({f"type_{t}_reads_zero": (lambda t=t: _type_case(t)) for t in ZERO_TYPES})
INGEST_CASES["u16_at_odd_offset"] = _u16_case
INGEST_CASES.update({f"layout_{k}": (lambda k=k: _layout_case(k))
                     for k in ("ends_at_last_byte_f32", "ends_at_last_byte_f64", "ends_at_last_byte_u8",
                               "step_1024_far_end", "device_lead_1", "device_lead_2", "device_lead_3")})


# the calls of the shared-scratch sequence (pack_counts serves ingest, egress and integrate_cloud2's statistics)
def scratch_blob(n, seed):
    rng = np.random.default_rng(seed)
    x, y, z = xyz(rng, n)
    x, y = (0.5 * x).astype(F32), (0.5 * y).astype(F32)     # inside the 8 m map of the sequence
    if n > 10_000:
        return make_blob(x, y, z, point_step=12, rng=rng)
    return make_blob(x, y, z, intensity=rng.random(n), point_step=16, rng=rng)


SCRATCH_BLOBS = {"ingest_300000": lambda: scratch_blob(300_000, 90), "integrate_1000": lambda: scratch_blob(1000, 91),
                 "ingest_5": lambda: scratch_blob(5, 92)}
INGEST_CASES.update({f"scratch_{k}": (lambda b=b: b() + (None, 0)) for k, b in SCRATCH_BLOBS.items()})


def ingest_case(name):
    blob, lay, n, lead = INGEST_CASES[name]()
    if n is None:
        n = len(blob) // lay.point_step
    assert isinstance(lay, Layout) and len(blob) == n * lay.point_step
    return blob, lay, n, lead
