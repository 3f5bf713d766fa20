"""Clouds built to reach the parts of the outlier removal's k-NN search (fastdem_amd/csrc/fdm_knn.hpp, the grid rule in
fdm_engine_dem.inl) that a uniformly scattered cloud never reaches.  Test data: tests/test_dem_restate.py proves on the
CPU that every probe tells a search that stops a ring early from an exact one, tests/test_sor_edges_gpu.py holds the
engine to the brute force of tests/dem_restate.py on them.

A DESIGNED cloud has a search grid known by construction: the x / y bounding box is [0, E]^2 with E * E * per = n
(per = max(4, k / 2) points per column), so the column size is exactly 1, a point's column is floor(coordinate), the
last column (index E) holds the points at exactly E, and a query's margin is its distance to the nearest integer.
Coordinates are multiples of 1/64: every difference, square and sum among near points is exact.

A PROBE is a query with
  k - 1 near neighbours    stacked above it, 1/64 apart
  the true k-th neighbour  straight across one face of the query's column, in ring S (S = `ring`), a distance
                           d = (columns crossed) + (the query's distance to that face) + delta away
  a decoy                  inside the block of rings 0 .. S - 1, at d + 1/64 or just beyond: what a search that stops
                           after ring S - 1 holds as its k-th candidate
and nothing else within six columns (the fillers keep to columns at least six away, in x or in y, from every probe's
column).  By default the true neighbour is the nearest lattice point of ring S — on the boundary of its column across a
+ face (delta = 0), 1/64 inside it across a - face (delta = 1): d lies AT or just ABOVE the bound (S - 1 + margin) * h
when the face crossed is the query's nearest one, so a search that loosens the bound stops at ring S - 1 with the decoy.
delta = 63 puts the neighbour 1/64 BELOW the bound of ring S itself: served from that ring, and still the same answer
from a search that tightens the bound and walks on.  ring = 0 has k near neighbours and neither of the two; ring = 5 is
beyond the rings a query lane visits (kKnnShells = 4), so the query must take the brute-force queue.
"""
import functools

import numpy as np

import dem_restate as DR

F32 = np.float32
U = 64                                                               # lattice units per metre
CLEAR = 6                                                            # fillers keep this many columns from a probe's column
DIRS = {"x+": (1, 0), "x-": (-1, 0), "y+": (0, 1), "y-": (0, -1)}


class Probe:
    """qx, qy: the query, in lattice units (1/64).  face: the face the true k-th neighbour lies across.  ring: S.
    delta: lattice units from the boundary of ring S's column to the neighbour (None: the nearest lattice point)."""

    def __init__(self, name, qx, qy, face, ring, delta=None, decoy="xy"):
        self.name, self.qx, self.qy, self.face, self.ring, self.delta, self.decoy = name, qx, qy, face, ring, delta, decoy
        self.index = None                                            # the query's index in the cloud

    def __repr__(self):
        return f"{self.name}[q=({self.qx / U}, {self.qy / U}) {self.face} ring {self.ring}]"

    def column(self, E):
        return min(self.qx // U, E), min(self.qy // U, E)

    def points(self, k, E):
        """int64[m, 3] lattice coordinates: the query first."""
        q = np.array([self.qx, self.qy, 0], dtype=np.int64)
        if self.ring == 0:
            return np.array([q + (0, 0, c) for c in range(k + 1)])
        pts = [q + (0, 0, c) for c in range(k)]                      # the query and its k - 1 near neighbours
        ax, sg = (0, DIRS[self.face][0]) if DIRS[self.face][0] else (1, DIRS[self.face][1])
        col = int(self.column(E)[ax])
        # the first lattice coordinate inside column col + sg * ring, seen from the query
        if sg > 0:
            first = (col + self.ring) * U
            delta = 0 if self.delta is None else self.delta
        else:
            first = (col - self.ring + 1) * U - 1
            delta = 1 if self.delta is None else self.delta
            delta -= 1
        t = q.copy()
        t[ax] = first + sg * delta
        d = abs(int(t[ax]) - int(q[ax]))                             # the true k-th distance, lattice units
        assert d > k - 1, (self, d)                                  # farther than the near stack
        assert 0 <= t[ax] <= E * U, (self, t)
        pts.append(t)
        dec = None
        if self.decoy == "xy" and self.ring >= 2:                    # back by ring - 1 whole columns, then sideways
            back = (self.ring - 1) * U
            side = int(np.floor(np.sqrt(d * d - back * back))) + 1
            for sgn in (1, -1):
                c = q.copy()
                c[ax] -= sg * back
                c[1 - ax] += sgn * side
                inside = 0 <= c[0] <= E * U and 0 <= c[1] <= E * U
                near = abs(min(int(c[1 - ax]) // U, E) - int(self.column(E)[1 - ax])) <= self.ring - 1
                if inside and near:
                    dec = c
                    break
        if dec is None:                                              # below the query, in its own column
            dec = q - (0, 0, d + 1)
        assert ((dec - q) ** 2).sum() > d * d
        pts.append(dec)
        return np.array(pts)


class Designed:
    """A designed cloud: x, y, z float32 (read-only), E, k, the probes with their query's index."""

    def __init__(self, name, E, n, k, probes, seed):
        assert n * 1.0 == max(4.0, 0.5 * k) * E * E, (name, n, k, E)  # h = sqrt(per * E * E / n) = 1
        self.name, self.E, self.k, self.probes = name, E, k, probes
        rng = np.random.default_rng(seed)
        cols = [p.column(E) for p in probes]
        for i, a in enumerate(cols):
            for b in cols[:i]:
                assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 12 or E < 24, (name, a, b)
        g = np.arange(E)                                             # (the last column, E, holds only coordinate E)
        free_x = np.array([all(abs(c - a[0]) >= CLEAR for a in cols) for c in g])
        free_y = np.array([all(abs(c - a[1]) >= CLEAR for a in cols) for c in g])
        ok = free_x[:, None] | free_y[None, :]                       # [cx, cy]
        fx, fy = np.nonzero(ok)
        assert fx.size and free_x.any() and free_y.any(), name
        parts = [p.points(k, E) for p in probes]
        starts = np.cumsum([0] + [len(a) for a in parts])
        n_fill = n - int(starts[-1])
        assert n_fill >= 4 + fx.size, (name, n_fill)
        pick = np.concatenate([np.arange(fx.size), rng.integers(0, fx.size, n_fill - 4 - fx.size)])
        fill = np.stack([fx[pick] * U + rng.integers(0, U, pick.size), fy[pick] * U + rng.integers(0, U, pick.size),
                         rng.integers(0, U // 2 + 1, pick.size)], axis=1)
        # the bounding box: one point on each side of [0, E]^2, in a filler column
        cx0, cy0 = int(g[free_x][0]) * U + 7, int(g[free_y][0]) * U + 9
        box = np.array([[0, cy0, 3], [E * U, cy0, 5], [cx0, 0, 7], [cx0, E * U, 11]])
        lat = np.concatenate(parts + [fill, box])
        order = rng.permutation(n)
        where = np.empty(n, dtype=np.int64)
        where[order] = np.arange(n)                                  # lat[i] ends up at where[i]
        for p, s in zip(probes, starts):
            p.index = int(where[s])
        lat = lat[order]
        assert lat[:, :2].min() == 0 and lat[:, :2].max() == E * U
        self.x, self.y, self.z = (np.ascontiguousarray(lat[:, a].astype(F32) / F32(U)) for a in range(3))
        for a in (self.x, self.y, self.z):
            a.setflags(write=False)
        self.grid = (F32(1.0), E + 1, E + 1)
        assert DR.sor_grid(0.0, 0.0, E, E, n, k) == self.grid, name

    def xyz(self):
        return self.x, self.y, self.z


def lb2(s, margin, h=1.0):
    """The square the k-th squared distance must stay below for a lane to stop after ring s (fdm_knn.hpp), fp32."""
    lb = F32(F32(F32(F32(s) + F32(margin)) - F32(0.00390625)) * F32(h)) * F32(0.9999)
    return F32(F32(lb * lb) * F32(0.9999)) if lb > 0 else F32(0.0)


def kth_d2(c, q, k, s=None):
    """The k-th smallest squared distance from point q: over the whole cloud, or over rings 0 .. s of q's column."""
    x, y, z = c.xyz()
    d2 = ((x - x[q]) ** 2 + (y - y[q]) ** 2) + (z - z[q]) ** 2
    d2[q] = np.inf
    if s is not None:
        cx, cy = DR.knn_columns(x, 0.0, 1.0, c.E + 1), DR.knn_columns(y, 0.0, 1.0, c.E + 1)
        d2[np.maximum(np.abs(cx - cx[q]), np.abs(cy - cy[q])) > s] = np.inf
    return np.sort(d2)[k - 1]


def check_probe(c, p):
    """On the restatement alone: an exact search of probe p is served by ring p.ring and no earlier ring (or by the
    queue, ring 5), and a search that stops one ring early returns a different mean.  Returns the true mean."""
    x, y, z = c.xyz()
    k, q, E = c.k, p.index, c.E
    assert (x[q], y[q]) == (F32(p.qx) / F32(U), F32(p.qy) / F32(U))
    grid = (1.0, 0.0, 0.0, E + 1, E + 1)
    true = DR.knn_mean_distances_of(x, y, z, k, [q])[0]
    fx, fy = p.qx / U - p.column(E)[0], p.qy / U - p.column(E)[1]
    margin = max(0.0, min(fx, 1 - fx, fy, 1 - fy))
    if p.ring >= 1:
        early = DR.knn_mean_within_rings(x, y, z, k, q, p.ring - 1, *grid)
        assert early != true and np.isfinite(early), (p, early, true)          # the decoy is held, and it is farther
        assert kth_d2(c, q, k, p.ring - 1) >= lb2(p.ring - 1, margin), p        # the rule itself must not stop there
    if p.ring <= 4:
        assert DR.knn_mean_within_rings(x, y, z, k, q, p.ring, *grid) == true, p
        p.stops_at = min(s for s in range(p.ring, 6) if s == 5 or kth_d2(c, q, k) < lb2(s, margin))
        assert p.stops_at <= 4, p                                               # served by a ring, not by the queue
        to_face = {"x+": 1 - fx, "x-": fx, "y+": 1 - fy, "y-": fy}[p.face]
        if to_face == margin:                                                   # across the nearest face: that very ring
            assert p.stops_at == p.ring, p
    else:
        assert kth_d2(c, q, k, 4) >= lb2(4, margin), p                          # ring 5: the lane must queue itself
        p.stops_at = None
    return true


# ---- the stopping rule, k = 8: [0, 64]^2, 16 384 points, 65 x 65 columns of 1 m --------------------------------------
SLOTS = (0, 13, 26, 38, 51, 64)                                      # probe columns: 12 or 13 apart, both borders


def _inner(cx, cy, face, margin64):
    """The query in column (cx, cy) whose nearest face is `face`, margin64 / 64 away; the other axis at mid-column."""
    ax, sg = (0, DIRS[face][0]) if DIRS[face][0] else (1, DIRS[face][1])
    off = [U // 2, U // 2]
    off[ax] = U - margin64 if sg > 0 else margin64
    return cx * U + off[0], cy * U + off[1]


def stopping_probes():
    P = []
    inner = [(a, b) for a in SLOTS[1:5] for b in SLOTS[1:5]]         # 16 interior slots
    # rings 1 .. 4 x the four nearest faces, the margins 1/64, 16/64 and 31/64 taken in turn: just above the bound
    plan = [(1, "x-", 16), (1, "x+", 31), (1, "y-", 16), (1, "y+", 31),
            (2, "x-", 1), (2, "x+", 16), (2, "y-", 31), (2, "y+", 1),
            (3, "x-", 31), (3, "x+", 1), (3, "y-", 16), (3, "y+", 31),
            (4, "x-", 16), (4, "x+", 31), (4, "y-", 1), (4, "y+", 16)]
    for (cx, cy), (ring, face, m) in zip(inner, plan):
        P.append(Probe(f"r{ring}{face}m{m}", *_inner(cx, cy, face, m), face, ring,
                       decoy="z" if (ring + m) % 2 else "xy"))
    # the border columns.  West (column 0): the nearest face is the grid's own border, the neighbour lies across
    # another; east (column 64): the clamped column of the points at exactly max_x, margin 0
    Em, mid = 64 * U, U // 2
    P += [Probe("west-r0", 16, SLOTS[1] * U + mid, "x+", 0),
          Probe("west-r5", 16, SLOTS[2] * U + mid, "x+", 5),                   # queued
          Probe("west-r3-below", 16, SLOTS[3] * U + mid, "x+", 3, delta=63),   # just below the bound of ring 3
          Probe("west-r2y", 31, SLOTS[4] * U + 16, "y-", 2),
          Probe("east-r1", Em, SLOTS[1] * U + mid, "x-", 1, delta=20),
          Probe("east-r4", Em, SLOTS[2] * U + mid, "x-", 4),
          Probe("east-r2y", Em, SLOTS[3] * U + 31, "y-", 2),
          Probe("east-r5", Em, SLOTS[4] * U + mid, "x-", 5),                   # queued
          Probe("south-r0", SLOTS[1] * U + mid, 31, "y+", 0),
          Probe("south-r4-below", SLOTS[2] * U + 48, 16, "x+", 4, delta=63),
          Probe("south-r5", SLOTS[3] * U + mid, 1, "y+", 5),                   # queued
          Probe("south-r1", SLOTS[4] * U + 33, 16, "x-", 1, delta=20),
          Probe("north-r3", SLOTS[1] * U + mid, Em, "y-", 3),
          Probe("north-r2-below", SLOTS[2] * U + 16, Em, "y-", 2, delta=63),
          Probe("north-r1x", SLOTS[3] * U + 16, Em, "x-", 1, delta=20),
          Probe("north-r4", SLOTS[4] * U + mid, Em, "y-", 4),
          Probe("corner-sw-r3", 16, mid, "x+", 3),
          Probe("corner-se-r4", Em, 16, "y+", 4),
          Probe("corner-nw-r2", 31, Em, "x+", 2),
          Probe("corner-ne-r5", Em, Em, "x-", 5)]                              # queued
    return P


def stopping_probes_2():
    """The second [0, 64]^2 cloud: ring 0 for every face, the inner ring 5, and both sides of the bound at rings 1 .. 4."""
    P = []
    inner = [(a, b) for a in SLOTS[1:5] for b in SLOTS[1:5]]
    plan = [(0, "x-", 16, None), (0, "x+", 31, None), (0, "y-", 31, None), (0, "y+", 16, None),
            (5, "x-", 16, None), (5, "y+", 1, None), (5, "x+", 31, None), (5, "y-", 16, None),
            (1, "x+", 16, 63), (2, "y-", 16, 63), (3, "x-", 31, 63), (4, "y+", 1, 63),     # just below the bound of ring S
            (2, "x+", 16, 0), (3, "y+", 31, 0), (4, "x+", 1, 0), (5, "y+", 16, 0)]         # AT the bound of ring S - 1
    for (cx, cy), (ring, face, m, delta) in zip(inner, plan):
        P.append(Probe(f"r{ring}{face}m{m}d{delta}", *_inner(cx, cy, face, m), face, ring, delta=delta,
                       decoy="xy" if (ring + m) % 2 else "z"))
    return P


# ---- the four top-k buckets at their edges: centre, border and one queued probe each ---------------------------------
def bucket_probes(E, variant):
    mid, c = U // 2, E // 2
    if E >= 24:                                                      # 33 x 33 columns: slots 0, 16, 32
        return [Probe("centre-r5", c * U + 16, c * U + mid, "x-", 5),
                Probe("west-r3", 16, c * U + mid, "x+", 3),
                Probe("east-r2", E * U, c * U + mid, "x-", 2),
                Probe("south-r4", c * U + mid, 16, "y+", 4),
                Probe("north-r2", c * U + 48, E * U, "y-", 2),
                Probe("corner-sw-r2", 31, 31, "y+", 2),
                Probe("corner-ne-r3", E * U, E * U, "x-", 3)]
    if variant == "a":                                               # 17 x 17 columns: two probes a cloud
        return [Probe("centre-r4", c * U + 48, c * U + mid, "x+", 4), Probe("corner-sw-r2", 16, 16, "x+", 2)]
    return [Probe("centre-r5", c * U + mid, c * U + 16, "y-", 5), Probe("corner-ne-r2", E * U, E * U, "y-", 2)]


BUCKETS = {  # name: (E, n, k, variant)
    "k4": (32, 4096, 4, ""), "k5": (32, 4096, 5, ""), "k16": (32, 8192, 16, ""), "k17": (32, 8704, 17, ""),
    "k32a": (16, 4096, 32, "a"), "k32b": (16, 4096, 32, "b"), "k33a": (16, 4224, 33, "a"), "k33b": (16, 4224, 33, "b"),
    "k64a": (16, 8192, 64, "a"), "k64b": (16, 8192, 64, "b")}


@functools.lru_cache(maxsize=None)
def designed(name):
    seed = 100                                                       # (no mean within 16 ulp of the threshold: checked per cloud)
    if name == "rings":
        return Designed(name, 64, 16384, 8, stopping_probes(), seed)
    if name == "rings2":
        return Designed(name, 64, 16384, 8, stopping_probes_2(), seed)
    E, n, k, variant = BUCKETS[name]
    return Designed(name, E, n, k, bucket_probes(E, variant), seed)


DESIGNED = ("rings", "rings2") + tuple(BUCKETS)


def whole_grid_exit():
    """[0, 8]^2, 256 points, k = 8: 9 x 9 columns of 1 m.  255 points crowd the four corners ([0, 1) and [7.75, 8]), one
    sits at (4.5, 4.5): every other point is at least 4.59 m from it, beyond the bound of ring 4 (4.5 m), and ring 4 is
    the whole grid — only the whole-cloud exit keeps it off the queue.  Returns x, y, z and the centre's index."""
    rng = np.random.default_rng(21)
    lat = [[4 * U + 32, 4 * U + 32, 0]]
    far = 7 * U + 48
    for i, (ox, oy) in enumerate(((0, 0), (far, 0), (0, far), (far, far))):
        m = 63 if i == 0 else 64
        pts = np.stack([ox + rng.integers(0, U if ox == 0 else 17, m), oy + rng.integers(0, U if oy == 0 else 17, m),
                        rng.integers(0, 33, m)], axis=1)
        pts[0] = [0 if ox == 0 else 8 * U, 0 if oy == 0 else 8 * U, 0]          # the box's corner itself
        lat += pts.tolist()
    lat = np.array(lat, dtype=np.int64)
    order = rng.permutation(256)
    lat = lat[order]
    x, y, z = (np.ascontiguousarray(lat[:, a].astype(F32) / F32(U)) for a in range(3))
    assert DR.sor_grid(0.0, 0.0, 8.0, 8.0, 256, 8) == (F32(1.0), 9, 9)
    return x, y, z, int(np.flatnonzero(order == 0)[0])


# ---- k_knn_brute at its edges, the grid rule's branches, scale --------------------------------------------------------
def lattice_cloud(n, seed, span, zspan=0.5, centre=(0.0, 0.0)):
    """n points on multiples of 1/64: x, y within span of the centre, z in [0, zspan]."""
    rng = np.random.default_rng(seed)
    q = int(span * U)
    x = rng.integers(-q, q + 1, n).astype(F32) / F32(U) + F32(centre[0])
    y = rng.integers(-q, q + 1, n).astype(F32) / F32(U) + F32(centre[1])
    z = rng.integers(0, int(zspan * U) + 1, n).astype(F32) / F32(U)
    return x, y, z


SPHERE = [(sx * a, sy * b, sz * c) for a, b, c in ((9, 12, 0), (12, 9, 0), (9, 0, 12), (12, 0, 9), (0, 9, 12),
                                                   (0, 12, 9), (15, 0, 0), (0, 15, 0), (0, 0, 15))
          for sx in ((1, -1) if a else (1,)) for sy in ((1, -1) if b else (1,)) for sz in ((1, -1) if c else (1,))]
DUP_FULL, DUP_FEW, TIE_CENTRE = (24.0, 24.0, 1.0), (-24.0, 24.0, 0.5), (25.0, -25.0, 0.0)


def _cat(*clouds):
    return tuple(np.ascontiguousarray(np.concatenate([c[a] for c in clouds]).astype(F32)) for a in range(3))


def _pts(rows):
    a = np.array(rows, dtype=F32)
    return a[:, 0], a[:, 1], a[:, 2]


def cloud(name):
    """(x, y, z, k) of a named case."""
    if name in ("ends50+150", "ends30+70"):                          # two clusters at the ends of a line, k = 64
        a, b = (50, 150) if name == "ends50+150" else (30, 70)
        rng = np.random.default_rng(31 + a)
        x = np.concatenate([rng.integers(0, 33, a), 16 * U - rng.integers(0, 33, b)])
        x[0], x[a] = 0, 16 * U
        y = rng.integers(0, 33, a + b)
        y[0], y[a] = 0, 32
        z = rng.integers(0, 33, a + b)
        return x.astype(F32) / F32(U), y.astype(F32) / F32(U), z.astype(F32) / F32(U), 64
    if name == "brute-sites":                                        # k = 10: three sites tens of metres from 3 000 points
        bulk = lattice_cloud(3000, 41, span=4.0)
        full = _pts([DUP_FULL] * 16)                                 # an isolated point and k + 5 copies of it
        few = _pts([DUP_FEW] * 5)                                    # five copies: six more neighbours are in the bulk
        cx, cy, cz = TIE_CENTRE
        tie = _pts([TIE_CENTRE] + [(cx + a, cy + b, cz + c) for a, b, c in SPHERE])   # 30 points exactly 15 m away
        return _cat(bulk, full, few, tie) + (10,)
    if name == "strip":                                              # the 2 048-column cap: 511.75 m x 1/16 m, k = 8
        rng = np.random.default_rng(51)
        n = 4000
        x = rng.integers(0, 2047 * 16 + 1, n)                        # multiples of 1/64 in [0, 511.75]
        x[:8], x[8:16], x[16:24] = rng.integers(0, 16, 8), 2047 * 16, 2046 * 16 + rng.integers(0, 16, 8)
        x[0] = 0
        y = rng.integers(0, 5, n)
        y[0], y[8] = 0, 4
        z = rng.integers(0, 17, n)
        return x.astype(F32) / F32(U), y.astype(F32) / F32(U), z.astype(F32) / F32(U), 8
    if name in ("line-x", "line-y"):                                 # a box without area: points per length
        rng = np.random.default_rng(52)
        a = rng.integers(0, 16 * U + 1, 300)
        a[:2] = 0, 16 * U
        a = a.astype(F32) / F32(U)
        b = np.full(300, 3.0, dtype=F32)
        z = rng.integers(0, 33, 300).astype(F32) / F32(U)
        return (a, b, z, 10) if name == "line-x" else (b, a, z, 10)
    if name == "pole":                                               # all x, y equal: one column
        rng = np.random.default_rng(53)
        z = rng.integers(0, 20 * U, 200).astype(F32) / F32(U)
        return np.full(200, -2.5, dtype=F32), np.full(200, 7.25, dtype=F32), z, 10
    if name == "one-point":                                          # one point, 20 times
        return np.full(20, 1.5, dtype=F32), np.full(20, -0.75, dtype=F32), np.full(20, 0.25, dtype=F32), 10
    if name == "two-corners":                                        # 2 x 2 000 points in opposite corners of 60 m x 60 m
        return _cat(lattice_cloud(2000, 56, span=0.75, centre=(-29.25, -29.25)),
                    lattice_cloud(2000, 57, span=0.75, centre=(29.25, 29.25))) + (10,)
    if name == "utm":                                                # a large common offset: the fp32 lattice is 1/32 m, 1/2 m
        rng = np.random.default_rng(61)
        return ((4.0e5 + rng.uniform(0, 60, 3000)).astype(F32), (5.0e6 + rng.uniform(0, 60, 3000)).astype(F32),
                rng.normal(0.0, 0.3, 3000).astype(F32), 10)
    if name == "arbitrary":                                          # tests/test_sor_gpu.py's cloud of arbitrary fp32
        rng = np.random.default_rng(12)
        return (rng.normal(3.0, 5.0, 2000).astype(F32), rng.normal(-7.0, 5.0, 2000).astype(F32),
                rng.normal(0.0, 0.3, 2000).astype(F32), 10)
    raise KeyError(name)


BIG_N, BIG_K, BIG_SAMPLE = 700001, 10, 512
BIG_PLANTED = (5, 123456, 350000, 600000, 699990)                    # points lifted tens of metres off the surface


def big_cloud():
    """700 001 points of arbitrary fp32 coordinates on a rolling surface of 260 m x 260 m (ten a square metre)."""
    rng = np.random.default_rng(71)
    x = rng.uniform(-130.0, 130.0, BIG_N)
    y = rng.uniform(-130.0, 130.0, BIG_N)
    z = 2.0 * np.sin(x / 17.0) * np.cos(y / 23.0) + rng.normal(0.0, 0.03, BIG_N)
    z[list(BIG_PLANTED)] += (30.0, 45.0, 60.0, -40.0, 35.0)
    return x.astype(F32), y.astype(F32), z.astype(F32)


def big_sample(x, y):
    """At least 512 query indices: the first and the last point, the extremes of x and of y, the planted points, the
    rest drawn by seed."""
    must = [0, BIG_N - 1, int(np.argmin(x)), int(np.argmax(x)), int(np.argmin(y)), int(np.argmax(y))] + list(BIG_PLANTED)
    rest = np.random.default_rng(72).permutation(BIG_N)[:BIG_SAMPLE]
    return np.unique(np.concatenate([np.array(must, dtype=np.int64), rest]))
