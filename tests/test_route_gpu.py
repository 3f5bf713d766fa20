"""Scan routing for a spatially tiled GLOBAL map (fdm_route.hpp, tiling.RoutedScan) against the ORACLE, in one process.

Every rank's tile engine lives in this process on device 0; the test does the exchange itself with device copies, by the
rules of tiling.RoutedScan.integrate: shares concatenated in source rank order, SoA shares padded to 4 points,
any_in_map = OR of every slice's n_in_map, and in sensors mode the same obstacle-clear skip rule.  No torch.distributed,
no child processes, so every plan of 1 .. 16 ranks runs on one GPU.

  * route kernels against a plain reference: the oracle's cell ids (c * rows + r, -1 cropped, -2 outside the map) give
    every point's owner through the plan's edges; numpy builds the stable partition (AoS records or SoA channel blocks
    at 4 * base[d] with pad4 strides) and the counters, and the device `send` buffer must match bit for bit: random
    slices, float32 points within 3 ulp of every owner edge (at the origin and 33 / 37 km out at 0.15 m), NaN / Inf /
    cropped points, slices outside the map or owned by the last rank, an empty first call, and slices of 2^21, 2^21 + 1
    and 2.7 M points (k_route_scan's second pass, buffer growth, stale rows);
  * routed streams end to end: 8, 16 and 5 tile engines with a 6-cell halo, slices mode and sensors mode, after every
    scan the counters against the oracle's statistics and every stored window against the oracle's map after a halo
    exchange through fdm_engine_regions_pack / unpack, and the four stencils on the final tiles;
  * regions_pack / unpack with more than 8 rectangles and more than 24 layers (several launches);
  * routing refuses an engine with raycasting on (its ray stage would only see its own share).

Run on the GPU box:  python -m pytest tests/test_route_gpu.py -m gpu
"""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_arrays_close
from test_batch_gpu import T

F32 = np.float32
GLOBAL, KALMAN, P2 = 1, 0, 1
SENSOR_Z = 1.2
HALO = 6
TILED_MIN = 1500   # (default variant) shares from this size up take the owners' tiled path

# id: (length_x, length_y, resolution, position, (rows, cols))
MAPS = {
    "sq": (15.7, 20.3, 0.1, (0.0, 0.0), (157, 203)),
    "far": (23.55, 30.45, 0.15, (-33333.3, 37777.7), (157, 203)),
    "strip": (120.1, 3.7, 0.1, (0.0, 0.0), (1201, 37)),
}


# ------------------------------------------------------------------------------------------ reference ----
def owners_of(ids, rows, row_edge, col_edge):
    """Owner rank of every point from its oracle cell id (-1 where the point lands in no cell).  row_edge / col_edge:
    the plan's pr + 1 / pc + 1 edges; rank i * pc + j owns rows [row_edge[i], row_edge[i+1]) x cols [col_edge[j], ...)."""
    ids = np.asarray(ids, dtype=np.int64)
    inside = ids >= 0
    r, c = ids % rows, ids // rows
    pc = len(col_edge) - 1
    i = np.searchsorted(np.asarray(row_edge[1:-1]), r, side="right")
    j = np.searchsorted(np.asarray(col_edge[1:-1]), c, side="right")
    return np.where(inside, i * pc + j, -1)


def pad4(v):
    return (np.asarray(v, dtype=np.int64) + 3) // 4 * 4


def expected_route(ids, rows, row_edge, col_edge, world, x, y, z, intensity, soa):
    """What fdm_engine_route_scan[_soa] must leave: counts (world + 2: per owner, n_after_filter, n_in_map), the base
    offset of every owner's share (in points; soa: sums of pad4(count)), and the partition as a list of
    (float offset into send, float32 values) segments covering exactly the defined part of the buffer."""
    ids = np.asarray(ids)
    own = owners_of(ids, rows, row_edge, col_edge)
    cnt = np.bincount(own[own >= 0], minlength=world)[:world]
    counts = np.concatenate([cnt, [int((ids != -1).sum()), int((ids >= 0).sum())]]).astype(np.int64)
    sizes = pad4(cnt) if soa else cnt
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    a = np.zeros(len(ids), F32) if intensity is None else np.asarray(intensity, F32)
    segs = []
    for d in range(world):
        sel = np.flatnonzero(own == d)   # stable: scan order inside every share
        if soa:
            P = int(pad4(cnt[d]))
            for ch, v in enumerate((x, y, z, a)):
                segs.append((4 * int(base[d]) + ch * P, np.asarray(v, F32)[sel]))
        else:
            rec = np.stack([np.asarray(v, F32)[sel] for v in (x, y, z, a)], axis=1)
            segs.append((4 * int(base[d]), rec.reshape(-1)))
    return counts, base, segs


def test_reference_partition_on_a_hand_written_example():
    """(no GPU) The numpy builder above on 3 owners (a 1 x 3 plan of a 4 x 6 grid) and 12 points."""
    rows = 4
    row_edge, col_edge = [0, 4], [0, 2, 4, 6]
    # cell id c * rows + r: columns 0-1 -> owner 0, 2-3 -> owner 1, 4-5 -> owner 2
    ids = [9, 0, -1, 22, 5, -2, 13, 1, 20, 12, -1, 7]
    #      1  0   .  2  0   .   1  0   2   1   .  0
    x = np.arange(12, dtype=F32) + F32(0.5)
    y, z, a = -x, 2 * x, 10 * x
    counts, base, segs = expected_route(ids, rows, row_edge, col_edge, 3, x, y, z, a, soa=False)
    assert counts.tolist() == [4, 3, 2, 10, 9]
    assert base.tolist() == [0, 4, 7]
    flat = np.concatenate([s for _, s in segs]).reshape(-1, 4)
    assert flat[:, 0].tolist() == [1.5, 4.5, 7.5, 11.5, 0.5, 6.5, 9.5, 3.5, 8.5]
    assert np.array_equal(flat[:, 3], 10 * flat[:, 0]) and np.array_equal(flat[:, 1], -flat[:, 0])
    counts, base, segs = expected_route(ids, rows, row_edge, col_edge, 3, x, y, z, None, soa=True)
    assert base.tolist() == [0, 4, 8]   # pad4(4) = 4, pad4(3) = 4
    offs = [o for o, _ in segs]
    assert offs == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44]   # owner 2: P = 4, at float 4 * 8
    assert segs[4][1].tolist() == [0.5, 6.5, 9.5] and segs[7][1].tolist() == [0.0, 0.0, 0.0]   # no intensity: 0
    assert segs[9][1].tolist() == [-3.5, -8.5]


# ------------------------------------------------------------------------------------------ plumbing ----
class FdmRegion(C.Structure):   # fdm_region (include/fdm_engine.h)
    _fields_ = [("r0", C.c_int32), ("c0", C.c_int32), ("nr", C.c_int32), ("nc", C.c_int32), ("offset", C.c_uint64)]


def regions_call(eng, rects, names, buf, pack):
    arr = (FdmRegion * len(rects))(*[FdmRegion(*r) for r in rects])
    nm = (C.c_char_p * len(names))(*[n.encode() for n in names])
    fn = eng._lib.fdm_engine_regions_pack if pack else eng._lib.fdm_engine_regions_unpack
    rc = fn(eng._h, len(rects), C.cast(arr, C.c_void_p), nm, len(names), C.c_void_p(buf.data_ptr()))
    assert rc == 0, eng._lib.fdm_last_error().decode()


def cfg_fill(est=KALMAN, ray=0):
    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 4.0, 0.2, 1.0e6
        c.mode, c.estimation_type, c.raycast_enabled = GLOBAL, est, ray
        return c
    return fill


def make_ref(R, gid, est=KALMAN):
    lx, ly, res, pos, shape = MAPS[gid]
    ref = R.RefEngine(lx, ly, res, cfg_fill(est)(R.default_config()), position=pos)
    assert (ref.rows, ref.cols) == shape
    ref.enable_cell_ids()
    return ref


def make_engine(gpu, gid, tile=None, est=KALMAN, ray=0):
    lx, ly, res, pos, shape = MAPS[gid]
    eng = gpu.Engine(lx, ly, res, cfg_fill(est, ray)(gpu.capi.default_config()), position=pos, tile=tile)
    assert (eng.rows, eng.cols) == shape
    return eng


def edges_of(rp):
    pr, pc = rp.grid_rows, rp.grid_cols
    return [rp.row_edge[k] for k in range(pr + 1)], [rp.col_edge[k] for k in range(pc + 1)]


def plans_for(world, shape):
    from fastdem_amd import tiling
    plans = [tiling.make_plan(r, world, shape[0], shape[1], HALO) for r in range(world)]
    return plans, tiling.route_plan(plans[0])


def edge_points(ref, row_edge, col_edge, rng, ulps=3, copies=4):
    """float32 coordinates within `ulps` ulp of every row and column edge of the plan (map borders included), the
    other coordinate at `copies` random cells of the map; identity transforms take them to getIndex unchanged."""
    g = ref.geometry()
    hx, hy, res = g.length_x / 2.0, g.length_y / 2.0, g.resolution
    xs, ys = [], []

    def around(v):
        f = F32(v)
        out, lo, hi = [f], f, f
        for _ in range(ulps):
            lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
            out += [lo, hi]
        return out

    def other(n, center, half, size):
        k = rng.integers(0, size, n)
        return (center + half - (k + rng.uniform(0.05, 0.95, n)) * res).astype(F32)
    for _ in range(copies):
        for k in row_edge:   # x of the edge between rows k - 1 and k: -(((x - half) - center) / res) == k
            v = around(g.position_x + hx - k * res)
            xs += v
            ys += list(other(len(v), g.position_y, hy, g.cols))
        for k in col_edge:
            v = around(g.position_y + hy - k * res)
            ys += v
            xs += list(other(len(v), g.position_x, hx, g.rows))
    for kr in row_edge:   # both coordinates on edges (corners of the owned rects)
        for kc in col_edge:
            for vx, vy in zip(around(g.position_x + hx - kr * res), around(g.position_y + hy - kc * res)[::-1]):
                xs.append(vx)
                ys.append(vy)
    x, y = np.asarray(xs, F32), np.asarray(ys, F32)
    return {"x": x, "y": y, "z": np.zeros_like(x)}


def mixed_points(ref, rng, n, intensity=True):
    """Random points over the map and a margin around it (every wavefront mixes owners), with NaN / Inf coordinates,
    points the crops drop (too high, too close to the sensor at the origin) and points outside the map."""
    g = ref.geometry()
    x = (g.position_x + rng.uniform(-0.55, 0.55, n) * g.length_x).astype(F32)
    y = (g.position_y + rng.uniform(-0.55, 0.55, n) * g.length_y).astype(F32)
    z = rng.uniform(-1.0, 1.0, n).astype(F32)
    pick = rng.integers(0, 40, n)
    x[pick == 0] = np.nan
    y[pick == 1] = np.inf
    x[pick == 2] = -np.inf
    z[pick == 3] = np.nan
    z[pick == 4] = 9.0          # above z_max
    x[pick == 5], y[pick == 5] = 0.05, -0.05   # inside range_min of the sensor at the origin
    s = {"x": x, "y": y, "z": z}
    if intensity:
        s["intensity"] = rng.uniform(0, 1, n).astype(F32)
    return s


def owned_by_last(ref, rp, rng, n):
    """n points inside the owned rect of the last rank."""
    g = ref.geometry()
    re, ce = edges_of(rp)
    r = rng.integers(re[-2], re[-1], n)
    c = rng.integers(ce[-2], ce[-1], n)
    x = (g.position_x + g.length_x / 2 - (r + rng.uniform(0.1, 0.9, n)) * g.resolution).astype(F32)
    y = (g.position_y + g.length_y / 2 - (c + rng.uniform(0.1, 0.9, n)) * g.resolution).astype(F32)
    return {"x": x, "y": y, "z": np.zeros(n, F32), "intensity": rng.uniform(0, 1, n).astype(F32)}


def oracle_ids(ref, s):
    n = int(s["x"].size)
    I4 = np.eye(4)
    rc, st = ref.integrate(s["x"], s["y"], s["z"], I4, I4, intensity=s.get("intensity"))
    ids = ref.last_cell_ids(n) if n else np.zeros(0, np.int32)
    return ids, st


class Router:
    """One routing engine plus its device buffers; route() checks a slice against the reference."""

    def __init__(self, gpu, eng, rp, world, rows):
        import torch
        self.torch, self.eng, self.rp, self.world, self.rows = torch, eng, rp, world, rows
        self.re, self.ce = edges_of(rp)

    def route(self, s, ids, soa, stats=None):
        torch, W = self.torch, self.world
        n = int(s["x"].size)
        dev = {c: torch.from_numpy(np.ascontiguousarray(s[c])).cuda() for c in ("x", "y", "z", "intensity") if c in s}
        send = torch.full((n + 3 * W + 4, 4), float("nan"), dtype=torch.float32, device="cuda")
        counts = torch.full((W + 2,), -7, dtype=torch.int32, device="cuda")
        if n == 0:
            dev = {c: torch.empty(0, dtype=torch.float32, device="cuda") for c in ("x", "y", "z")}
        self.eng.route_scan(self.rp, dev["x"], dev["y"], dev["z"], np.eye(4), np.eye(4), send, counts,
                            intensity=dev.get("intensity"), soa=soa)
        self.eng.sync()
        got_counts = counts.cpu().numpy().astype(np.int64)
        want_counts, base, segs = expected_route(ids, self.rows, self.re, self.ce, W, s["x"], s["y"], s["z"],
                                                 s.get("intensity"), soa)
        assert got_counts.tolist() == want_counts.tolist(), (soa, got_counts, want_counts)
        if stats is not None:   # the reference reading of the ids is the oracle's own statistics
            assert (want_counts[W], want_counts[W + 1]) == (stats["n_after_filter"], stats["n_in_map"]), stats
        flat = send.view(-1).cpu().numpy()
        for off, want in segs:
            got = flat[off:off + want.size]
            bad = got.view(np.uint32) != want.view(np.uint32)
            assert not bad.any(), f"soa={soa}: {int(bad.sum())} of {want.size} floats differ at send[{off}:]"
        return got_counts


# ------------------------------------------------------------------------------ (a) route kernels ----
ROUTE_CASES = [(w, "sq") for w in (1, 2, 3, 5, 6, 8, 12, 16)] + \
              [(w, "far") for w in (2, 5, 8, 16)] + [(w, "strip") for w in (3, 5, 8, 16)]


@pytest.fixture(scope="module")
def fa():
    """fastdem_amd with a usable device (the route kernels do not depend on the engines' pipeline options)."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import fastdem_amd
    fastdem_amd.capi.load()
    return fastdem_amd


@pytest.mark.gpu
@pytest.mark.parametrize("world,gid", ROUTE_CASES, ids=[f"w{w}_{g}" for w, g in ROUTE_CASES])
def test_route_kernels_against_the_oracle_cells(fa, R, world, gid):
    shape = MAPS[gid][4]
    plans, rp = plans_for(world, shape)
    ref = make_ref(R, gid)
    rng = np.random.default_rng(world * 131 + len(gid))
    # the routing engine: the last rank's tile (routing uses the GLOBAL geometry whatever the tile)
    eng = make_engine(fa, gid, tile=plans[-1].fdm_tile() if world > 1 else None)
    rt = Router(fa, eng, rp, world, shape[0])
    empty = {"x": np.zeros(0, F32), "y": np.zeros(0, F32), "z": np.zeros(0, F32)}
    c = rt.route(empty, np.zeros(0, np.int32), soa=bool(world % 2))   # the first call on a fresh engine
    assert not c.any()
    g = ref.geometry()
    outside = mixed_points(ref, rng, 3000)
    outside["x"] += F32(2.0 * g.length_x)
    slices = [mixed_points(ref, rng, int(rng.integers(3000, 9000))),
              mixed_points(ref, rng, 777, intensity=False),
              edge_points(ref, *edges_of(rp), rng),
              outside,
              owned_by_last(ref, rp, rng, 1029)]
    for k, s in enumerate(slices):
        ids, st = oracle_ids(ref, s)
        if k == 2:
            r = ids[ids >= 0] % shape[0]
            for e in edges_of(rp)[0][1:-1]:   # every interior row edge has points on both sides
                assert (r == e - 1).any() and (r == e).any(), e
        if k == 3:
            assert st["n_in_map"] == 0 and st["n_after_filter"] > 0
        for soa in (False, True):
            c = rt.route(s, ids, soa, st)
        if k == 4:
            assert c[world - 1] == s["x"].size and c[:world - 1].sum() == 0


@pytest.mark.gpu
def test_route_kernels_on_slices_beyond_one_scan_pass(fa, R):
    """k_route_scan walks the block counts 8192 blocks (2^21 points) per pass: slices of 2^21, 2^21 + 1 and 2.7 M
    points (a second pass, and buffer growth), then a smaller slice (stale rows beyond its blocks)."""
    world = 16
    shape = MAPS["sq"][4]
    plans, rp = plans_for(world, shape)
    ref = make_ref(R, "sq")
    rng = np.random.default_rng(2024)
    big = mixed_points(ref, rng, 2_700_001)
    ids, st = oracle_ids(ref, big)
    eng = make_engine(fa, "sq", tile=plans[5].fdm_tile())
    rt = Router(fa, eng, rp, world, shape[0])
    for n, soa in ((2_097_152, False), (2_097_153, True), (2_700_001, False), (2_700_001, True), (300_001, True),
                   (2_097_153, False), (299_999, False)):
        s = {c: v[:n] for c, v in big.items()}
        rt.route(s, ids[:n], soa, st if n == 2_700_001 else None)


# -------------------------------------------------------------- (c) regions_pack / unpack chunking ----
@pytest.mark.gpu
def test_regions_pack_unpack_more_than_8_rects_and_24_layers(fa, R):
    rng = np.random.default_rng(77)
    plans, _ = plans_for(8, MAPS["sq"][4])
    tile = plans[5].fdm_tile()
    a, b = make_engine(fa, "sq", tile=tile), make_engine(fa, "sq", tile=tile)
    s = mixed_points(make_ref(R, "sq"), rng, 20000)
    for e in (a, b):
        e.integrate(s["x"], s["y"], s["z"], np.eye(4), np.eye(4), intensity=s["intensity"])
    user = [f"user_{k}" for k in range(20)]
    for e in (a, b):
        for nm in user:
            e.add(nm)
    names = user[:13] + [n for n in a.layers() if not n.startswith("user_")] + user[13:]
    assert len(names) > 24, names
    sr, sc = a.s_rows, a.s_cols
    for nm in names:
        for e in (a, b):
            v = rng.normal(0, 1, (sr, sc)).astype(F32)
            v[rng.uniform(size=v.shape) < 0.1] = np.nan
            v[rng.uniform(size=v.shape) < 0.05] = -0.0
            e.set_layer(nm, v)
    # eleven disjoint rectangles (some 1 x n, n x 1), blocks at offsets with gaps between them
    rects, off = [], 3
    cols = np.linspace(0, sc, 12).astype(int)
    for q in range(11):
        c0, c1 = int(cols[q]), int(cols[q + 1])
        r0 = int(rng.integers(0, sr // 2))
        nr = 1 if q == 3 else int(rng.integers(1, sr - r0))
        nc = 1 if q == 7 else c1 - c0
        rects.append((r0, c0, nr, nc, off))
        off += nr * nc * len(names) + int(rng.integers(1, 40))
    import torch
    sentinel = -12345.5
    buf = torch.full((off + 8,), sentinel, dtype=torch.float32, device="cuda")
    regions_call(a, rects, names, buf, pack=True)
    a.sync()
    got = buf.cpu().numpy()
    covered = np.zeros(got.size, bool)
    la = {nm: a.layer(nm) for nm in names}
    for r0, c0, nr, nc, o in rects:
        cells = nr * nc
        for l, nm in enumerate(names):
            blk = got[o + l * cells:o + (l + 1) * cells].reshape(nc, nr).T   # column-major inside the block
            want = la[nm][r0:r0 + nr, c0:c0 + nc]
            assert np.array_equal(blk.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (nm, r0, c0)
            covered[o + l * cells:o + (l + 1) * cells] = True
    assert (got[~covered] == sentinel).all(), "pack wrote outside the rectangles' blocks"
    lb = {nm: b.layer(nm) for nm in names}
    regions_call(b, rects, names, buf, pack=False)
    b.sync()
    for nm in names:
        want = lb[nm].copy()
        for r0, c0, nr, nc, o in rects:
            want[r0:r0 + nr, c0:c0 + nc] = la[nm][r0:r0 + nr, c0:c0 + nc]
        assert np.array_equal(b.layer(nm).view(np.uint32), want.view(np.uint32)), nm


# ---------------------------------------------------------------------------- (d) raycasting ----
@pytest.mark.gpu
def test_routing_refuses_an_engine_with_raycasting(fa, R):
    """An owner's ray stage would see only its own share while rays from the rest of the scan cross its cells: the
    routed path cannot reproduce the single map's ghost removal, so route_scan refuses such an engine."""
    import torch
    plans, rp = plans_for(8, MAPS["sq"][4])
    eng = make_engine(fa, "sq", tile=plans[2].fdm_tile(), ray=1)
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    send = torch.empty((64 + 3 * 8 + 4, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros(10, dtype=torch.int32, device="cuda")
    for soa in (False, True):
        with pytest.raises(fa.engine.EngineError, match="raycast"):
            eng.route_scan(rp, x, x, x, np.eye(4), np.eye(4), send, counts, soa=soa)
    ok = make_engine(fa, "sq", tile=plans[2].fdm_tile(), ray=0)
    ok.route_scan(rp, x, x, x, np.eye(4), np.eye(4), send, counts)
    ok.sync()


# ------------------------------------------------------------------ (b) routed streams end to end ----
class TiledMap:
    """`world` tile engines (6-cell halo) of one GLOBAL map, driven by the rules of tiling.RoutedScan, next to the oracle."""

    def __init__(self, gpu, R, gid, world, est):
        import torch
        self.torch, self.gid, self.world = torch, gid, world
        self.shape = MAPS[gid][4]
        self.plans, self.rp = plans_for(world, self.shape)
        self.ref = make_ref(R, gid, est)
        self.ref.enable_cell_ids(False)
        self.tiles = [make_engine(gpu, gid, tile=p.fdm_tile(), est=est) for p in self.plans]
        if "tiled_min" not in gpu.Engine.default_options:
            for t in self.tiles:
                t.set_option("tiled_min", TILED_MIN)
        self.dirty = [True] * world   # (sensors mode) the tile's obstacle layer may hold non-NaN cells
        self.integrated = 0           # owner calls that carried points

    def _route(self, r, s, Tbs, Twb, soa):
        torch, W = self.torch, self.world
        n = int(s["x"].size)
        d = {c: torch.from_numpy(np.ascontiguousarray(s[c])).cuda() for c in ("x", "y", "z", "intensity") if c in s}
        send = torch.empty((n + 3 * W + 4, 4), dtype=torch.float32, device="cuda")
        counts = torch.zeros(W + 2, dtype=torch.int32, device="cuda")
        self.tiles[r].route_scan(self.rp, d["x"], d["y"], d["z"], Tbs, Twb, send, counts, intensity=d.get("intensity"),
                                 soa=soa)
        return send, counts, d

    def step_slices(self, s, Tbs, Twb, align):
        from fastdem_amd import tiling
        torch, W = self.torch, self.world
        n = int(s["x"].size)
        outs = [self._route(r, {c: v[lo:hi] for c, v in s.items()}, Tbs, Twb, False)
                for r, (lo, hi) in enumerate(tiling.slice_bounds(n, W, align))]
        for t in self.tiles:
            t.sync()
        m = np.stack([c.cpu().numpy().astype(np.int64) for _, c, _ in outs])
        base = np.concatenate([np.zeros((W, 1), np.int64), np.cumsum(m[:, :W], axis=1)[:, :-1]], axis=1)
        any_in_map = bool(m[:, W + 1].sum() > 0)
        keep = []
        for dst in range(W):
            parts = [outs[src][0][base[src, dst]:base[src, dst] + m[src, dst]] for src in range(W)]
            recv = torch.cat(parts) if m[:, dst].sum() else torch.empty((0, 4), dtype=torch.float32, device="cuda")
            keep.append(recv)
            self.tiles[dst].integrate_points4_device(recv, int(m[:, dst].sum()), Tbs, Twb,
                                                     has_intensity="intensity" in s, any_in_map=any_in_map)
            self.integrated += int(m[:, dst].sum() > 0)
        for t in self.tiles:
            t.sync()
        rc, st = self.ref.integrate(s["x"], s["y"], s["z"], Tbs, Twb, intensity=s.get("intensity"))
        assert n == st["n_input"] or n == 0
        assert (int(m[:, :W].sum()), int(m[:, W].sum()), int(m[:, W + 1].sum())) == \
            (st["n_in_map"], st["n_after_filter"], st["n_in_map"]), (m.sum(axis=0), st)
        return st

    def step_sensors(self, scans):
        """scans[r] = (points, Tbs, Twb) of rank r: the step is W integrate() calls in rank order."""
        W = self.world
        outs = [self._route(r, s, Tbs, Twb, True) for r, (s, Tbs, Twb) in enumerate(scans)]
        for t in self.tiles:
            t.sync()
        m = np.stack([c.cpu().numpy().astype(np.int64) for _, c, _ in outs])
        base = np.concatenate([np.zeros((W, 1), np.int64), np.cumsum(pad4(m[:, :W]), axis=1)[:, :-1]], axis=1)
        for dst in range(W):
            for src in range(W):
                ns = int(m[src, dst])
                seen = bool(m[src, W + 1] > 0)
                if ns == 0 and not (seen and self.dirty[dst]):
                    continue   # tiling.RoutedScan's rule: nothing for this tile and its obstacle layer is clear already
                s, Tbs, Twb = scans[src]
                share = outs[src][0].view(-1)[4 * int(base[src, dst]):]
                self.tiles[dst].integrate_soa4_device(share, ns, Tbs, Twb, has_intensity="intensity" in s,
                                                      any_in_map=seen)
                self.dirty[dst] = ns > 0
                self.integrated += int(ns > 0)
        for t in self.tiles:
            t.sync()
        for src, (s, Tbs, Twb) in enumerate(scans):
            rc, st = self.ref.integrate(s["x"], s["y"], s["z"], Tbs, Twb, intensity=s.get("intensity"))
            assert (int(m[src, :W].sum()), int(m[src, W]), int(m[src, W + 1])) == \
                (st["n_in_map"], st["n_after_filter"], st["n_in_map"]), (src, m[src], st)
            assert int(s["x"].size) == st["n_input"] or s["x"].size == 0

    def names(self):
        common = set(self.tiles[0].layers())
        for t in self.tiles[1:]:
            common &= set(t.layers())
        return sorted(common)

    def exchange(self):
        """Halo exchange: one regions_pack per tile for all its send strips, device copies into one receive buffer per
        tile (blocks a few floats apart), one regions_unpack per tile."""
        torch, names = self.torch, self.names()
        L = len(names)
        if not names:
            return names
        packed, where = [], {}
        for t, p in enumerate(self.plans):
            rects, off = [], 5
            for o in sorted(p.sends):
                rc = p.sends[o]
                loc = rc.local_to(p.stored)
                rects.append((loc.r0, loc.c0, loc.nr, loc.nc, off))
                where[(t, o)] = (off, L * rc.nr * rc.nc)
                off += L * rc.nr * rc.nc + 3
            buf = torch.empty(off, dtype=torch.float32, device="cuda")
            if rects:
                regions_call(self.tiles[t], rects, names, buf, pack=True)
            packed.append(buf)
        for t in self.tiles:
            t.sync()
        recvs = []
        for t, p in enumerate(self.plans):
            rects, off, parts = [], 2, []
            for o in sorted(p.recvs):
                rc = p.recvs[o]
                loc = rc.local_to(p.stored)
                so, ln = where[(o, t)]
                rects.append((loc.r0, loc.c0, loc.nr, loc.nc, off))
                parts.append((off, so, ln, o))
                off += ln + 7
            buf = torch.full((off,), float("nan"), dtype=torch.float32, device="cuda")
            for ro, so, ln, o in parts:
                buf[ro:ro + ln].copy_(packed[o][so:so + ln])
            torch.cuda.synchronize()
            if rects:
                regions_call(self.tiles[t], rects, names, buf, pack=False)
            recvs.append(buf)
        for t in self.tiles:
            t.sync()
        return names

    def compare(self, what):
        ref_names = self.ref.layers()
        full = {nm: self.ref.layer(nm) for nm in ref_names}
        common = set(self.names())
        for t, p in zip(self.tiles, self.plans):
            have = t.layers()
            assert set(have) <= set(ref_names), (what, have, ref_names)
            st, ow = p.stored, p.owned
            for nm in ref_names:
                if nm not in have:   # no point with that channel reached this tile
                    assert np.isnan(full[nm][ow.r0:ow.r1, ow.c0:ow.c1]).all(), (what, p.rank, nm)
                    continue
                # the stored window (the ring too) where every tile holds the layer; the owned window otherwise
                win = st if nm in common else ow
                got = t.layer(nm)[win.r0 - st.r0:win.r1 - st.r0, win.c0 - st.c0:win.c1 - st.c0]
                want = full[nm][win.r0:win.r1, win.c0:win.c1]
                na, nb = np.isnan(got), np.isnan(want)
                if nm == "color":
                    na = nb = np.zeros_like(na)
                assert np.array_equal(na, nb), f"{what}: rank {p.rank} {nm}: NaN pattern differs in {(na != nb).sum()}"
                bad = got.view(np.uint32)[~na] != want.view(np.uint32)[~nb]
                assert not bad.any(), f"{what}: rank {p.rank} {nm}: {int(bad.sum())} cells differ in their bits"

    def stencils(self, R):
        res = MAPS[self.gid][2]

        def run(o):
            o.apply_uncertainty_fusion(True, 6 * res, 2 * res, 0.05, 0.95, 3)   # 6 cells
            o.apply_inpainting(3, 2)                                          # 3 cells
            o.apply_spatial_smoothing("elevation_inpainted", 5, 5)            # 2 more
            o.apply_feature_extraction(6 * res, 4, 0.05, 0.95)                # 6 cells
        R.set_trig_mode(1)
        try:
            for o in [self.ref] + self.tiles:
                run(o)
        finally:
            R.set_trig_mode(0)
        for t in self.tiles:
            t.sync()
        n_checked = 0
        for nm in self.ref.layers():
            full = self.ref.layer(nm)
            for t, p in zip(self.tiles, self.plans):
                st, ow = p.stored, p.owned
                want = full[ow.r0:ow.r1, ow.c0:ow.c1]
                if not t.exists(nm):
                    assert np.isnan(want).all(), (p.rank, nm)
                    continue
                got = t.layer(nm)[ow.r0 - st.r0:ow.r1 - st.r0, ow.c0 - st.c0:ow.c1 - st.c0]
                assert_arrays_close(got, want, f"rank {p.rank} {nm}", 0.0, 0.0)
                n_checked += int(np.isfinite(want).sum())
        return n_checked


def ground(rng, n, lx, ly):
    """n points in the sensor frame of a pose near the map's centre: ground at z 0 +- 0.5 m over the map and a margin."""
    return {"x": rng.uniform(-lx / 2 - 0.5, lx / 2 + 0.5, n).astype(F32),
            "y": rng.uniform(-ly / 2 - 0.5, ly / 2 + 0.5, n).astype(F32),
            "z": (rng.uniform(-0.5, 0.5, n) - SENSOR_Z).astype(F32)}


class Stream:
    """The seeded scan stream of one run (numpy Generator: the stream is the test's definition)."""

    TBS = T(0.0, 0.0, SENSOR_Z)

    def __init__(self, tm, seed):
        self.tm, self.rng = tm, np.random.default_rng(seed)
        lx, ly, res, pos, _ = MAPS[tm.gid]
        self.lx, self.ly, self.res, self.pos = lx, ly, res, pos

    def size(self, big_ok=True):
        pick = int(self.rng.integers(0, 10))
        if pick < 4:
            return int(self.rng.integers(1, 400))
        if pick < 7 or not big_ok:
            return int(self.rng.integers(900, 3500))
        return int(self.rng.integers(20000, 50000))

    def scan(self, k, kind, n, intensity):
        """(points, T_base_sensor, T_world_base) of one logical scan."""
        r = self.rng
        px, py = self.pos
        yaw = float(r.uniform(-np.pi, np.pi))
        if kind == "edges":   # identity transforms: the coordinates reach getIndex unchanged
            s = edge_points(self.tm.ref, *edges_of(self.tm.rp), r)
            s["z"] = r.uniform(-0.5, 0.5, s["x"].size).astype(F32)
            Tbs = Twb = np.eye(4)
        elif kind == "patch":   # inside the owned rect of one tile: every other owner gets nothing
            p = self.tm.plans[int(r.integers(0, self.tm.world))].owned
            g = self.tm.ref.geometry()
            cr, cc = p.r0 + p.nr / 2.0, p.c0 + p.nc / 2.0
            ex = g.position_x + g.length_x / 2 - cr * g.resolution
            ey = g.position_y + g.length_y / 2 - cc * g.resolution
            half = 0.3 * min(p.nr, p.nc) * g.resolution
            s = {"x": r.uniform(-half, half, n).astype(F32), "y": r.uniform(-half, half, n).astype(F32),
                 "z": (r.uniform(-0.5, 0.5, n) - SENSOR_Z).astype(F32)}
            Tbs, Twb = self.TBS, T(ex, ey, 0.0)
        else:
            s = ground(r, n, self.lx, self.ly)
            dx, dy = float(r.uniform(-0.1, 0.1) * self.lx), float(r.uniform(-0.1, 0.1) * self.ly)
            if kind == "outside":
                dx += 3.0 * self.lx
            if kind == "filtered":
                s["z"] += F32(20.0)
            Tbs, Twb = self.TBS, T(px + dx, py + dy, 0.0, yaw=yaw if kind != "outside" else 0.0)
            if kind == "wide":   # undo the yaw on the points so that the cloud still spans the map
                c, sn = np.cos(-yaw), np.sin(-yaw)
                s["x"], s["y"] = (c * s["x"] - sn * s["y"]).astype(F32), (sn * s["x"] + c * s["y"]).astype(F32)
        if intensity:
            s["intensity"] = r.uniform(0, 1, s["x"].size).astype(F32)
        return s, Tbs, Twb

    def kind(self, k, specials):
        if k in specials:
            return specials[k]
        return "patch" if int(self.rng.integers(0, 4)) == 0 else "wide"


# id: (map, world, estimator)
STREAMS = {
    "w8_2x4": ("sq", 8, KALMAN),
    "w16_4x4_far": ("far", 16, P2),
    "w5_1x5_strip": ("strip", 5, KALMAN),
}
N_SCANS = 36
INTENSITY_FROM = 14   # the intensity layer is created lazily mid-stream


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["slices", "sensors"])
@pytest.mark.parametrize("sid", sorted(STREAMS))
def test_routed_stream_against_the_oracle(gpu, R, sid, mode):
    """A seeded stream of routed scans into `world` tile engines: after every scan the counters equal the oracle's
    statistics and, after a halo exchange through regions_pack / unpack, every stored window equals the oracle's map
    bit for bit; at the end the stencils on every tile equal the oracle's on the owned cells."""
    gid, world, est = STREAMS[sid]
    tm = TiledMap(gpu, R, gid, world, est)
    sm = Stream(tm, seed=world * 1000 + (7 if mode == "sensors" else 3))
    specials = {0: "patch", 3: "outside", 5: "filtered", 9: "patch", 20: "outside"}
    if gid == "sq":
        specials[7] = specials[25] = "edges"
    in_map = 0
    for k in range(N_SCANS):
        inten = k >= INTENSITY_FROM and int(sm.rng.integers(0, 5)) > 0
        if mode == "slices":
            kind = sm.kind(k, specials)
            s, Tbs, Twb = sm.scan(k, kind, sm.size(), inten)
            st = tm.step_slices(s, Tbs, Twb, align=int(sm.rng.choice([1, 4])))
            if kind in ("outside", "filtered"):
                assert st["n_in_map"] == 0, (k, kind, st)
            in_map += st["n_in_map"]
        else:
            scans = []
            for r in range(world):
                kind = sm.kind(k, specials) if r == k % world else \
                    ("empty" if int(sm.rng.integers(0, 6)) == 0 else sm.kind(-1, {}))
                if kind == "empty":
                    scans.append(({c: np.zeros(0, F32) for c in ("x", "y", "z")}, Stream.TBS, T()))
                    continue
                scans.append(sm.scan(k, kind, sm.size(big_ok=(r + k) % 5 == 0), inten))
            tm.step_sensors(scans)
        tm.exchange()
        tm.compare(f"{sid} {mode} scan {k}")
    assert tm.integrated > 2 * N_SCANS, "the owners must have integrated routed points"
    assert {"intensity", "elevation", "obstacle"} <= set(tm.ref.layers())
    assert tm.stencils(R) > 1000
