"""Plain NumPy restatement of fastdem/io/pcd_convert.hpp, written from fastdem/src/pcd_convert.cpp and not from the engine
— the reading the engine's fromPointCloud / toPointCloud are held to (tests/test_raster_gpu.py); its own known answers
are in tests/test_raster_restate.py.  Test data, not product.

  restate_raster       fromPointCloud(cloud, map, method)         pcd_convert.cpp:29-153
  restate_auto_geometry fromPointCloud(cloud, resolution, method)  :155-181 (the geometry arithmetic)
  restate_to_cloud     toPointCloud(map)                          :327-373

A point's cell comes from the oracle's grid (`grid.get_index(x, y)` -> (ok, (row, col)): start index and edges are the
oracle's business, tests/test_oracle_grid.py).  Welford runs point by point in np.float32 scalars, per cell, in input
order.
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
METHODS = ("max", "min", "mean", "minmax")          # RasterMethod, in the enum's order
BASIC_LAYERS = ["elevation", "elevation_min", "elevation_max"]   # ElevationMap's constructor


class CellStats:                                      # BatchCellStats :32-59
    def __init__(self):
        self.mean, self.m2 = F32(0.0), F32(0.0)
        self.min_z, self.max_z = F32(FLT_MAX), F32(-FLT_MAX)
        self.count = 0
        self.max_intensity = F32(-FLT_MAX)
        self.last_color = np.uint32(0)
        self.has_intensity = self.has_color = False

    def add_z(self, z):                               # :44-53
        z = F32(z)
        self.count += 1
        with np.errstate(all="ignore"):
            delta = F32(z - self.mean)
            self.mean = F32(self.mean + F32(delta / F32(self.count)))
            delta2 = F32(z - self.mean)
            self.m2 = F32(self.m2 + F32(delta * delta2))
        if z < self.min_z:
            self.min_z = z
        if z > self.max_z:
            self.max_z = z

    def variance(self):                               # :56-58
        with np.errstate(all="ignore"):
            return F32(0.0) if self.count < 2 else F32(self.m2 / F32(self.count - 1))


def welford(values):
    """(mean, variance, count) of fp32 `values` applied in the given order."""
    s = CellStats()
    for v in np.asarray(values, dtype=F32):
        s.add_z(v)
    return s.mean, s.variance(), s.count


def restate_raster(grid, layers, order, x, y, z, intensity=None, rgb=None, method="max"):
    """Applies the cloud to `layers` (name -> float32[rows, cols], modified in place; `order` = getLayers(), extended in
    place).  Returns the list of layer names written (empty: nothing happened), in the order :114-151 touches them."""
    assert method in METHODS
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    if x.size == 0:                                   # :65
        return []
    has_intensity, has_color = intensity is not None, rgb is not None
    cells = {}
    for i in range(x.size):                           # :74-101
        if np.isnan(z[i]):
            continue
        ok, rc = grid.get_index(float(x[i]), float(y[i]))   # nanogrid::Position(pt.x(), pt.y()): float -> double
        if not ok:
            continue
        s = cells.setdefault(rc, CellStats())
        s.add_z(z[i])
        if has_intensity:
            val = F32(intensity[i])
            if (not s.has_intensity) or val > s.max_intensity:
                s.max_intensity, s.has_intensity = val, True
        if has_color:
            s.last_color, s.has_color = np.uint32(int(rgb[i]) & 0x00FFFFFF), True   # colorVectorToValue: r<<16 | g<<8 | b
    if not cells:                                     # :103
        return []
    shape = next(iter(layers.values())).shape

    def ensure(name, value):                          # :106-112
        if name not in layers:
            layers[name] = np.full(shape, value, dtype=F32)
            order.append(name)

    ensure("elevation_min", np.nan)
    ensure("elevation_max", np.nan)
    ensure("variance", np.nan)
    ensure("n_points", 0.0)
    if has_intensity:
        ensure("intensity", np.nan)
    if has_color:
        ensure("color", np.nan)
    for (r, c), s in cells.items():                   # :121-152
        layers["elevation"][r, c] = {"max": s.max_z, "min": s.min_z, "mean": s.mean, "minmax": s.max_z}[method]
        layers["elevation_min"][r, c] = s.min_z
        layers["elevation_max"][r, c] = s.max_z
        layers["variance"][r, c] = s.variance()
        layers["n_points"][r, c] = F32(s.count)
        if has_intensity and s.has_intensity:
            layers["intensity"][r, c] = s.max_intensity
        if has_color and s.has_color:
            layers["color"].view(np.uint32)[r, c] = s.last_color
    return (["elevation", "elevation_min", "elevation_max", "variance", "n_points"] +
            (["intensity"] if has_intensity else []) + (["color"] if has_color else []))


def restate_auto_geometry(x, y, resolution):
    """(length_x, length_y, resolution, position_x, position_y, rows, cols) as Python floats (doubles) / ints, or None
    for an empty cloud (:157)."""
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    if x.size == 0:
        return None
    res = F32(resolution)
    keep = ~(np.isnan(x) | np.isnan(y))               # :167
    min_x = min_y = F32(FLT_MAX)
    max_x = max_y = F32(-FLT_MAX)
    if keep.any():                                    # std::min / std::max over non-NaN values
        min_x, max_x = min(min_x, x[keep].min()), max(max_x, x[keep].max())
        min_y, max_y = min(min_y, y[keep].min()), max(max_y, y[keep].max())
    with np.errstate(all="ignore"):
        width = F32(F32(max_x - min_x) + res)         # :175-176, float
        height = F32(F32(max_y - min_y) + res)
        px = np.float64(F32(min_x + max_x)) / 2.0     # :181: float sum, double divide
        py = np.float64(F32(min_y + max_y)) / 2.0
    # ElevationMap::setGeometry(float, float, float) -> nanogrid: size = round(length / resolution), length = size * res
    r64 = np.float64(res)
    rows, cols = int(np.round(np.float64(width) / r64)), int(np.round(np.float64(height) / r64))
    return (float(rows * r64), float(cols * r64), float(r64), float(px), float(py), rows, cols)


def restate_to_cloud(layers, geometry):
    """dict x, y, z (float32), intensity (float32 or None), rgb (uint32 or None).

    layers    name -> float32[rows, cols] indexed by BUFFER row / column
    ASSUMED visiting order of map.cells(): what the packed-cloud egress uses for the whole map — unwrapped column by
    unwrapped column from the start index, rows fastest (tests/io_restate.py restate_pack)."""
    g = geometry
    rows, cols = int(g.rows), int(g.cols)
    res = np.float64(g.resolution)
    origin_x = np.float64(g.position_x) + np.float64(g.length_x) / 2.0 - res / 2.0     # :335-338
    origin_y = np.float64(g.position_y) + np.float64(g.length_y) / 2.0 - res / 2.0
    jj, ii = np.meshgrid(np.arange(cols), np.arange(rows), indexing="ij")
    ur, uc = ii.reshape(-1), jj.reshape(-1)           # unwrapped row / col of every visit
    r, c = (ur + int(g.start_row)) % rows, (uc + int(g.start_col)) % cols
    z = layers["elevation"][r, c]
    keep = ~np.isnan(z)                               # :345
    out = {"x": (origin_x - ur[keep].astype(np.float64) * res).astype(F32),            # :347-348
           "y": (origin_y - uc[keep].astype(np.float64) * res).astype(F32),
           "z": z[keep].astype(F32), "intensity": None, "rgb": None}
    if "intensity" in layers:                         # :351-357
        a = layers["intensity"][r, c][keep]
        if (~np.isnan(a)).any():
            out["intensity"] = np.where(np.isnan(a), F32(0.0), a).astype(F32)
    if "color" in layers:                             # :359-369
        p = np.ascontiguousarray(layers["color"][r, c][keep])
        if (~np.isnan(p)).any():
            out["rgb"] = np.where(np.isnan(p), np.uint32(0), p.view(np.uint32) & np.uint32(0x00FFFFFF)).astype(np.uint32)
    return out


def order_sensitive_values(seed=7, n=4000):
    """n fp32 values from N(50, 30) whose Welford variance depends on the order they are applied in
    (tests/test_raster_restate.py asserts that it does)."""
    rng = np.random.default_rng(seed)
    return rng.normal(50.0, 30.0, n).astype(F32)
