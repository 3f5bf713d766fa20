"""Plain NumPy restatements of the two I/O stages, written from the reference's source and not from oracle/ — the
second reading that the engine AND the oracle are held to (tests/test_io_restate_vs_oracle.py on the CPU,
tests/test_egress_edges_gpu.py and tests/test_ingest_edges_gpu.py on the device).  Test data, not product.

  restate_pack        fastdem::detail::toPointCloud2Impl, fastdem/include/fastdem/bridge/ros/impl.hpp:28-166 (+ the
                      full-map overload :168-174, layer::isInternal elevation_map.hpp:42-45)
  restate_from_cloud2 nanopcl from_impl, fastdem/lib/nanoPCL/include/nanopcl/bridge/ros/impl.hpp:179-270, with
                      readIntensity :104-119 and readRgb :169-177
"""
import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------------- egress ----
def restate_pack(layers, order, geometry, elevation_layer="elevation", sub=None, window=None):
    """(fields, records float32[n, F]).

    layers     name -> float32[rows, cols] indexed by BUFFER row / column (what Engine.layer() returns); with
               `window` = (row0, col0, rows, cols) the arrays cover that window of the buffer only (a tiled engine
               stores nothing else and skips the cells outside it)
    order      getLayers() order
    geometry   rows, cols, start_row, start_col, position_x/_y, length_x/_y, resolution
    sub        (r0, c0, n_rows, n_cols) in buffer indices; None = the full-map overload
    """
    g = geometry
    rows, cols = int(g.rows), int(g.cols)
    start = (int(g.start_row), int(g.start_col))
    if sub is None:                                          # :168-174: sub_start = start index, sub_size = size
        sub = (start[0], start[1], rows, cols)
    r0, c0, sub_rows, sub_cols = (int(v) for v in sub)
    res = np.float64(g.resolution)
    origin_x = np.float64(g.position_x) + np.float64(g.length_x) / 2.0 - res / 2.0      # :43-46
    origin_y = np.float64(g.position_y) + np.float64(g.length_y) / 2.0 - res / 2.0

    def axis(first, count, size, start_index, origin):      # :48-64
        buf = (first + np.arange(count, dtype=np.int64)) % size
        unwrapped = (buf - start_index + size) % size
        coord = origin - unwrapped.astype(np.float64) * res  # int * double, double - double
        assert coord.dtype == np.float64
        return buf, coord.astype(F32)                        # static_cast<float>: one round-to-nearest-even

    buf_row, row_x = axis(r0, sub_rows, rows, start[0], origin_x)
    buf_col, col_y = axis(c0, sub_cols, cols, start[1], origin_y)

    float_layers = [n for n in order                         # :66-77
                    if not n.startswith("_") and n != elevation_layer and n != "color"]
    has_color = "color" in order
    fields = ["x", "y", "z"] + float_layers + (["rgb"] if has_color else [])      # :92-100

    # the visit: for j in sub_cols: for i in sub_rows  (:136-139) == the j-major flattening of the (j, i) grid
    jj, ii = np.meshgrid(np.arange(sub_cols), np.arange(sub_rows), indexing="ij")
    r, c = buf_row[ii.reshape(-1)], buf_col[jj.reshape(-1)]
    x, y = row_x[ii.reshape(-1)], col_y[jj.reshape(-1)]
    if window is not None:
        w_r0, w_c0, w_rows, w_cols = (int(v) for v in window)
        inside = (r >= w_r0) & (r < w_r0 + w_rows) & (c >= w_c0) & (c < w_c0 + w_cols)
        r, c, x, y = r[inside] - w_r0, c[inside] - w_c0, x[inside], y[inside]

    def bits(name):
        a = np.asarray(layers[name])
        assert a.dtype == F32, (name, a.dtype)
        return a[r, c].view(np.uint32) if a.size else np.zeros(0, np.uint32)

    z = bits(elevation_layer)
    keep = np.isfinite(z.view(F32))                          # :142
    out = np.empty((int(keep.sum()), len(fields)), dtype=np.uint32)
    out[:, 0], out[:, 1], out[:, 2] = x[keep].view(np.uint32), y[keep].view(np.uint32), z[keep]
    for k, name in enumerate(float_layers):                  # :152-156: memcpy of the float, bits as they are
        out[:, 3 + k] = bits(name)[keep]
    if has_color:                                            # :158-161
        out[:, -1] = bits("color")[keep]
    return fields, out.view(F32)


# ---------------------------------------------------------------------------------------------------- ingest ----
def restate_from_cloud2(blob, n, layout):
    """dict x, y, z (float32), intensity (float32 or None), rgb (uint32 0x00RRGGBB or None) of the kept points."""
    L = layout
    empty = {"x": np.zeros(0, F32), "y": np.zeros(0, F32), "z": np.zeros(0, F32), "intensity": None, "rgb": None}
    if n == 0:                                               # :184-187
        return empty
    if L.off_x < 0 or L.off_y < 0 or L.off_z < 0:            # :189-192
        return empty
    rec = np.frombuffer(blob, dtype=np.uint8, count=n * L.point_step).reshape(n, L.point_step)   # :231

    def field(off, dtype):
        size = np.dtype(dtype).itemsize
        return np.ascontiguousarray(rec[:, off:off + size]).view(dtype).reshape(n)

    x, y, z = (field(o, "<f4") for o in (L.off_x, L.off_y, L.off_z))                  # :233-235
    keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)                           # :238-240
    out = {"x": x[keep], "y": y[keep], "z": z[keep], "intensity": None, "rgb": None}
    if L.off_intensity >= 0:                                 # readIntensity :105-119
        t = L.intensity_type
        if t == 2:
            a = field(L.off_intensity, "u1").astype(F32)
        elif t == 4:
            a = field(L.off_intensity, "<u2").astype(F32)
        elif t == 7:
            a = field(L.off_intensity, "<f4")
        elif t == 8:
            with np.errstate(all="ignore"):
                a = field(L.off_intensity, "<f8").astype(F32)   # static_cast<float>(double): round to nearest even
        else:
            a = np.zeros(n, F32)
        out["intensity"] = a[keep]
    if L.off_rgb >= 0:                                       # readRgb :170-177: r, g, b = bits 16-23, 8-15, 0-7
        out["rgb"] = field(L.off_rgb, "<u4")[keep] & np.uint32(0x00FFFFFF)
    return out
