"""Plain NumPy restatement of fastdem::buildDEM and its two filters, written from the reference's sources and not from the
engine — the reading the engine's build_dem / statistical_outlier_removal / remove_floating_points are held to
(tests/test_sor_gpu.py, tests/test_build_dem_gpu.py); its own known answers are in tests/test_dem_restate.py.  Test
data, not product.

  restate_sor             nanopcl::filters::statisticalOutlierRemoval   outlier_removal_impl.hpp:83-142
  restate_ground_peak     findGroundPeak                                pcd_convert.cpp:194-220
  restate_floating        removeFloatingPoints                          pcd_convert.cpp:228-269
  restate_floating_grouped  the same mask by NumPy grouping, for clouds of 10^5 points (proved equal to the loop above in
                          tests/test_dem_restate.py); floating_cells / floating_bins: its cells and bin indices, which
                          the proofs of tests/dem_cases.py read
  restate_build_dem       buildDEM                                      pcd_convert.cpp:275-323

For tests/test_sor_edges_gpu.py (clouds built against the engine's column search, tests/sor_cases.py):
  knn_mean_distances_of   the brute-force means of a sample of queries (a cloud too large for every pair)
  knn_mean_within_rings   what a column search that stops after ring s would return: the wrong answer of a probe
  knn_columns, sor_grid   the search grid's columns and its size rule, restated

The k-NN is brute force (every pair), in fp32 with the reference's operation order ((dx*dx) + (dy*dy)) + (dz*dz); the two
global sums are SEQUENTIAL fp64 sums (np.cumsum: np.sum is pairwise and rounds differently).  A point's cell comes from
the oracle's grid, rasterization from tests/raster_restate.py, inpainting from the oracle as tests/test_post_gpu.py uses it.
"""
import numpy as np

import raster_restate as RR

F32 = np.float32
MAX_K = 64


def effective_k(n, k):
    """min(size_t(k), n - 1); 0 where the reference returns an empty cloud (:86-92)."""
    if n < 2 or k == 0:
        return 0
    return n - 1 if k < 0 else min(int(k), n - 1)    # a negative int converts to a huge size_t


def _knn_rows(x, y, z, k, rows):
    """The mean distances of the queries `rows` (indices into the cloud) against every point of the cloud."""
    dx = x[rows, None] - x[None, :]
    dy = y[rows, None] - y[None, :]
    dz = z[rows, None] - z[None, :]
    d2 = ((dx * dx) + (dy * dy)) + (dz * dz)                         # float32 throughout: one rounding per operation
    assert d2.dtype == F32
    d2[np.arange(rows.size), rows] = np.inf                          # only the query's own index is left out
    best = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
    root = np.sqrt(best)                                             # correctly rounded in fp32
    acc = np.zeros(rows.size, dtype=F32)
    for j in range(k):                                               # sum += sqrt(dist_sq), nearest first
        acc = (acc + root[:, j]).astype(F32)
    return acc / F32(k)


def knn_mean_distances(x, y, z, k, chunk=512):
    """float32[n]: (sum of sqrt of the k smallest squared distances to the OTHER points, ascending, fp32) / float(k)."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    n = x.size
    out = np.empty(n, dtype=F32)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        out[a:b] = _knn_rows(x, y, z, k, np.arange(a, b))
    return out


def knn_mean_distances_of(x, y, z, k, queries, cells=1 << 23):
    """float32[len(queries)]: knn_mean_distances' values at the point indices `queries`, by the same arithmetic, in
    chunks of about `cells` distances (a sample of a cloud too large for every pair)."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    queries = np.asarray(queries, dtype=np.int64)
    chunk = max(1, cells // max(1, x.size))
    out = np.empty(queries.size, dtype=F32)
    for a in range(0, queries.size, chunk):
        out[a:a + chunk] = _knn_rows(x, y, z, k, queries[a:a + chunk])
    return out


def knn_columns(p, mn, h, g):
    """The search grid's column of coordinates p along one axis, as fdm_knn.hpp's knn_col(knn_u(p, mn, 1 / h), g) has
    it: a subtraction and a multiplication rounded to fp32 each, truncation, the clamp to [0, g - 1]."""
    inv_h = F32(1.0) / F32(h)
    u = ((np.asarray(p, dtype=F32) - F32(mn)).astype(F32) * inv_h).astype(F32)
    return np.clip(u.astype(np.int64), 0, int(g) - 1)


def knn_mean_within_rings(x, y, z, k, q, s, h, min_x, min_y, gx, gy):
    """The mean distance point q would get from a search that looks no further than ring s: brute force over the points
    whose column lies within Chebyshev distance s of q's column (inf where these are fewer than k).  What a column
    search that stops after ring s returns — the wrong answer a probe is built to tell from the right one."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    cx, cy = knn_columns(x, min_x, h, gx), knn_columns(y, min_y, h, gy)
    near = np.flatnonzero(np.maximum(np.abs(cx - cx[q]), np.abs(cy - cy[q])) <= s)
    if near.size - 1 < k:
        return F32(np.inf)
    return _knn_rows(x[near], y[near], z[near], k, np.flatnonzero(near == q))[0]


def sor_grid(min_x, min_y, max_x, max_y, n, k, grid_max=2048):
    """(h, gx, gy) of the search grid: the arithmetic of fdm_engine_dem.inl's sor_grid, for test clouds that are built
    to reach one of its branches.  h in fp64 first (area rule, length rule, the column cap), then fp32."""
    ex, ey = float(F32(max_x)) - float(F32(min_x)), float(F32(max_y)) - float(F32(min_y))
    per = max(4.0, 0.5 * k)
    h = float(np.sqrt(per * ex * ey / n))
    if not h > 0.0:
        h = per * max(ex, ey) / n
    h = max(h, max(ex, ey) / (grid_max - 1))
    hf = F32(h)
    with np.errstate(divide="ignore", over="ignore"):
        inv = F32(1.0) / hf
    if not (hf > 0 and np.isfinite(hf) and np.isfinite(inv) and inv > 0):
        hf, inv = F32(1.0), F32(1.0)

    def cols(mx, mn):
        u = F32(F32(F32(mx) - F32(mn)) * inv)
        c = np.floor(float(u)) if np.isfinite(u) and u > 0 else 0.0
        return int(min(c, grid_max - 1)) + 1
    return hf, cols(max_x, min_x), cols(max_y, min_y)


def sor_threshold(mean, std_mul):
    """(:118-129) two sequential fp64 sums, then fp32."""
    m64 = mean.astype(np.float64)
    n = mean.size
    global_mean = np.cumsum(m64)[-1] / np.float64(n)
    diff = m64 - global_mean
    ss = np.cumsum(diff * diff)[-1]
    global_std = F32(np.sqrt(ss / np.float64(n)))
    return F32(F32(global_mean) + F32(F32(std_mul) * global_std))


def restate_sor(x, y, z, k, std_mul=1.0):
    """(keep bool[n], mean float32[n] or None, threshold float32 or None); None where no neighbour search happens."""
    n = np.asarray(x).size
    ke = effective_k(n, k)
    if ke == 0:
        return np.zeros(n, dtype=bool), None, None
    mean = knn_mean_distances(x, y, z, ke)
    thr = sor_threshold(mean, std_mul)
    return mean <= thr, mean, thr


def ulp_gap_to_threshold(mean, thr):
    """Smallest distance, in units of the threshold's ulp, between a mean distance and the threshold."""
    return float(np.min(np.abs(mean.astype(np.float64) - np.float64(thr))) / np.float64(np.spacing(F32(thr))))


def _int_cast(v):
    """static_cast<int>(float): truncation; out of range is undefined in C++ and an error here."""
    v = float(v)
    if not (-2147483649.0 < v < 2147483648.0):
        raise OverflowError("float does not fit an int")
    return int(v)


def restate_ground_peak(z_values, bin_size):
    """findGroundPeak: the centre of the LOWEST bin holding the largest count, fp32."""
    zs = np.asarray(z_values, dtype=F32)
    if zs.size == 0:
        return F32(0.0)
    b = F32(bin_size)
    z_min, z_max = zs.min(), zs.max()
    n_bins = max(1, _int_cast(F32(F32(z_max - z_min) / b)) + 1)
    counts = {}
    for v in zs:
        i = min(_int_cast(F32(F32(v - z_min) / b)), n_bins - 1)
        counts[i] = counts.get(i, 0) + 1
    best_bin, best_count = 0, 0
    for i in sorted(counts):                                         # ascending bins, strict '>'
        if counts[i] > best_count:
            best_count, best_bin = counts[i], i
    return F32(z_min + F32(F32(F32(best_bin) + F32(0.5)) * b))


def restate_floating(grid, x, y, z, height_threshold, bin_size):
    """removeFloatingPoints: keep bool[n]."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    cells = {}
    for i in range(x.size):
        if np.isnan(z[i]):
            continue
        ok, rc = grid.get_index(float(x[i]), float(y[i]))
        if ok:
            cells.setdefault(rc, []).append(i)
    keep = np.zeros(x.size, dtype=bool)
    for idx in cells.values():
        cutoff = F32(restate_ground_peak(z[idx], bin_size) + F32(height_threshold))
        for i in idx:
            if z[i] <= cutoff:
                keep[i] = True
    return keep


def floating_cells(grid, x, y, z):
    """int64[n]: the key (row << 32 | col) of the oracle's cell of every point, -1 where removeFloatingPoints skips the
    point (:236-241: a NaN z, no cell)."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    key = np.full(x.size, -1, dtype=np.int64)
    for i in np.flatnonzero(~np.isnan(z)):
        ok, (r, c) = grid.get_index(float(x[i]), float(y[i]))
        if ok:
            key[i] = (int(r) << 32) | int(c)
    return key


def floating_bins(key, z, bin_size):
    """(live, group, z_min, bins): the indices of the points that have a cell, the number of each one's cell among the
    distinct cells (ascending key), float32 z_min per cell, and int64 bin per live point — findGroundPeak's
    min(int((z - z_min) / bin), n_bins - 1) with n_bins = max(1, int((z_max - z_min) / bin) + 1), every operation rounded
    to fp32 as in restate_ground_peak; OverflowError where _int_cast raises."""
    z = np.asarray(z, dtype=F32)
    live = np.flatnonzero(key >= 0)
    uniq, group = np.unique(key[live], return_inverse=True)
    zl, b = z[live], F32(bin_size)
    z_min, z_max = np.full(uniq.size, np.inf, dtype=F32), np.full(uniq.size, -np.inf, dtype=F32)
    np.minimum.at(z_min, group, zl)
    np.maximum.at(z_max, group, zl)
    with np.errstate(all="ignore"):
        span = (z_max - z_min) / b
        at = (zl - z_min[group]) / b
    assert span.dtype == F32 and at.dtype == F32
    for v in (span, at):
        if not ((v > -2147483649.0) & (v < 2147483648.0)).all():     # a NaN too
            raise OverflowError("float does not fit an int")
    n_bins = np.maximum(1, span.astype(np.int64) + 1)                # astype: truncation, as static_cast<int>
    return live, group, z_min, np.minimum(at.astype(np.int64), n_bins[group] - 1)


def restate_floating_grouped(grid, x, y, z, height_threshold, bin_size, key=None):
    """restate_floating's mask, cell by cell in NumPy instead of point by point: the same fp32 operations in the same
    order per value.  `key`: floating_cells(grid, x, y, z) where the caller has it already."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    if key is None:
        key = floating_cells(grid, x, y, z)
    keep = np.zeros(x.size, dtype=bool)
    live, group, z_min, bins = floating_bins(key, z, bin_size)
    if live.size == 0:
        return keep
    # runs of equal (cell, bin); per cell the LOWEST bin among those with the largest count (:209-216, strict '>')
    order = np.lexsort((bins, group))
    g, b = group[order], bins[order]
    head = np.flatnonzero(np.r_[True, (g[1:] != g[:-1]) | (b[1:] != b[:-1])])
    count = np.diff(np.r_[head, g.size])
    rg, rb = g[head], b[head]
    pick = np.lexsort((rb, -count, rg))
    first = pick[np.r_[True, rg[pick][1:] != rg[pick][:-1]]]
    best = np.empty(z_min.size, dtype=np.int64)
    best[rg[first]] = rb[first]
    bs = F32(bin_size)
    with np.errstate(all="ignore"):
        ground = z_min + (best.astype(F32) + F32(0.5)) * bs          # :219
        cutoff = ground + F32(height_threshold)                      # :257
    assert ground.dtype == F32 and cutoff.dtype == F32
    keep[live] = z[live] <= cutoff[group]
    return keep


class DEM:
    """What restate_build_dem returns: geometry tuple (restate_auto_geometry), grid, layers in order, the stage counts."""

    def __init__(self):
        self.geometry = self.grid = None
        self.order, self.store = [], {}
        self.n_after_sor = self.n_after_height = 0
        self.threshold = None

    def layers(self):
        return list(self.order)

    def layer(self, name):
        return self.store[name]


def restate_build_dem(R, x, y, z, intensity=None, rgb=None, resolution=0.1, method="max", sor_k=10, sor_std_mul=1.0,
                      height_threshold=2.0, bin_size=0.0, inpaint_iterations=3, sor=None, floating=restate_floating):
    """A DEM, or None where the reference returns an uninitialised map (:276, :282).  `sor`: (keep, threshold) of the
    outlier removal where the caller has shown what it is without the k-NN search (a cloud too large for every pair);
    `floating`: restate_floating or restate_floating_grouped."""
    x, y, z = (np.asarray(v, dtype=F32) for v in (x, y, z))
    if x.size == 0:
        return None
    keep, thr = sor if sor is not None else restate_sor(x, y, z, sor_k, sor_std_mul)[::2]
    if not keep.any():
        return None
    sel = lambda a: None if a is None else np.asarray(a)[keep]       # noqa: E731
    x, y, z, intensity, rgb = x[keep], y[keep], z[keep], sel(intensity), sel(rgb)
    out = DEM()
    out.threshold, out.n_after_sor = thr, int(x.size)
    res = F32(resolution)
    geo = RR.restate_auto_geometry(x, y, res)                        # :285-305: the same arithmetic as :160-181
    out.geometry = geo
    out.grid = R.RefEngine(float(F32(geo[0])), float(F32(geo[1])), float(res), position=(geo[3], geo[4]))
    g = out.grid.geometry()
    assert (g.length_x, g.length_y, g.resolution, g.rows, g.cols) == (geo[0], geo[1], geo[2], geo[5], geo[6])
    b = F32(bin_size) if bin_size > 0 else res                       # :308-309
    keep2 = floating(out.grid, x, y, z, height_threshold, b)
    sel2 = lambda a: None if a is None else a[keep2]                 # noqa: E731
    x, y, z, intensity, rgb = x[keep2], y[keep2], z[keep2], sel2(intensity), sel2(rgb)
    out.n_after_height = int(x.size)
    out.order = list(RR.BASIC_LAYERS)
    out.store = {n: np.full((geo[5], geo[6]), np.nan, dtype=F32) for n in out.order}
    RR.restate_raster(out.grid, out.store, out.order, x, y, z, intensity, rgb, method)
    if inpaint_iterations > 0:                                       # :317-320: in place, on `elevation`
        out.grid.set_layer("elevation", out.store["elevation"])
        out.grid.apply_inpainting(int(inpaint_iterations), 2, True)
        out.store["elevation"] = np.array(out.grid.layer("elevation"), dtype=F32)
    return out
