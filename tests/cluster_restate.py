"""nanopcl::segmentation::euclideanCluster restated in NumPy / Python from what the reference does, step by step:
search::VoxelHash (its own open-addressing table: Fibonacci slot, linear probing, chains that grow at the head), the
radius search over (2 range + 1)^3 voxels, the BFS that grows a component from every unvisited seed in ascending index,
the size filter, the final sort by size — read as a STABLE sort — and the CSR.  Beside it a brute-force connected
components over the relation alone, and the canonical form the device is compared with.

fp32 throughout: inv = 1 / tol, voxel = floor(c * inv) (a product), r_sq = tol * tol, range = int(ceil(tol * inv)),
dist_sq = dx*dx + (dy*dy + dz*dz) — the three-term order the project fixes."""
import numpy as np

F = np.float32
COORD_OFFSET = 1 << 20
COORD_MIN, COORD_MAX = -COORD_OFFSET, COORD_OFFSET - 1
COORD_MASK = 0x1FFFFF
INVALID_KEY = (1 << 64) - 1
INVALID_INDEX = 0xFFFFFFFF
HASH_MULTIPLIER = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def relation_constants(tol):
    tol = F(tol)
    inv = F(1.0) / tol
    return inv, tol * tol, int(np.ceil(tol * inv))


def voxels(pts, inv):
    """floor(c * inv) per axis as int64 [m, 3] (an fp32 product)."""
    return np.floor(pts * F(inv)).astype(np.int64)


def dist_sq(a, b):
    """The fixed order: dx*dx + (dy*dy + dz*dz), every operation rounded to fp32.  a: [k, 3], b: [3] or [k, 3]."""
    d = (a - b).astype(F)
    s = d * d
    return s[..., 0] + (s[..., 1] + s[..., 2])


def _clamp(v):
    return min(max(v, COORD_MIN), COORD_MAX)


def pack(ix, iy, iz):
    ix, iy, iz = _clamp(ix), _clamp(iy), _clamp(iz)
    return ((iz + COORD_OFFSET) << 42) | ((iy + COORD_OFFSET) << 21) | (ix + COORD_OFFSET)


def unpack(key):
    return ((key & COORD_MASK) - COORD_OFFSET, ((key >> 21) & COORD_MASK) - COORD_OFFSET,
            ((key >> 42) & COORD_MASK) - COORD_OFFSET)


class VoxelHash:
    """search::VoxelHash(resolution): build(cloud) and radius(center, r)."""

    def __init__(self, resolution):
        self.inv = F(1.0) / F(resolution)

    def slot_of(self, key):
        return ((key * HASH_MULTIPLIER) & M64) >> self.shift

    def build(self, pts):
        n = pts.shape[0]
        self.pts = pts
        size = 1
        while size < 2 * n:
            size <<= 1
        self.keys = [INVALID_KEY] * size
        self.head = [INVALID_INDEX] * size
        self.next = [INVALID_INDEX] * n
        self.mask = size - 1
        self.shift = 64 - (size.bit_length() - 1)
        vox = voxels(pts, self.inv)
        finite = np.isfinite(pts).all(axis=1)
        for i in range(n):
            if not finite[i]:
                continue
            key = pack(int(vox[i, 0]), int(vox[i, 1]), int(vox[i, 2]))
            slot = self.slot_of(key)
            while True:
                if self.keys[slot] == INVALID_KEY:
                    self.keys[slot], self.head[slot], self.next[i] = key, i, INVALID_INDEX
                    break
                if self.keys[slot] == key:
                    self.next[i] = self.head[slot]
                    self.head[slot] = i
                    break
                slot = (slot + 1) & self.mask
        self._chains, self._near = {}, {}

    def chain(self, slot):
        """The slot's chain from its head on, as an array (walked once, then remembered: the table no longer changes)."""
        c = self._chains.get(slot)
        if c is None:
            out, idx = [], self.head[slot]
            while idx != INVALID_INDEX:
                out.append(idx)
                idx = self.next[idx]
            c = self._chains[slot] = np.asarray(out, dtype=np.int64)
        return c

    def candidates(self, center_key, rng):
        """The chains of the (2 rng + 1)^3 voxels around a centre voxel, joined in the order the reference's three loops
        and its probing reach them (found once per centre voxel, then remembered: the table no longer changes)."""
        c = self._near.get(center_key)
        if c is None:
            cx, cy, cz = unpack(center_key)
            found = []
            for dx in range(-rng, rng + 1):
                for dy in range(-rng, rng + 1):
                    for dz in range(-rng, rng + 1):
                        key = pack(cx + dx, cy + dy, cz + dz)
                        slot = self.slot_of(key)
                        while self.keys[slot] != INVALID_KEY:
                            if self.keys[slot] == key:
                                found.append(self.chain(slot))
                                break
                            slot = (slot + 1) & self.mask
            c = self._near[center_key] = np.concatenate(found) if found else np.zeros(0, dtype=np.int64)
        return c

    def radius(self, center, r):
        """The indices within r of `center`, in the order the reference's callback sees them."""
        r = F(r)
        r_sq = r * r
        rng = int(np.ceil(r * self.inv))
        cv = np.floor(center * self.inv).astype(np.int64)
        c = self.candidates(pack(int(cv[0]), int(cv[1]), int(cv[2])), rng)
        return c[dist_sq(self.pts[c], center) <= r_sq]


def cluster_core(pts, tolerance, min_size, max_size):
    """detail::clusterCore over the [m, 3] fp32 points: (clusters in the reference's order, each in BFS order; every
    component in seed order with its rejected ones, for the tests)."""
    m = pts.shape[0]
    if m == 0:
        return [], []
    search = VoxelHash(tolerance)
    search.build(pts)
    visited = np.zeros(m, dtype=bool)
    clusters, components = [], []
    for seed in range(m):
        if visited[seed]:
            continue
        queue, at = [seed], 0  # growCluster
        visited[seed] = True
        while at < len(queue):
            current = queue[at]
            at += 1
            nb = search.radius(pts[current], tolerance)
            new = nb[~visited[nb]]
            visited[new] = True
            queue.extend(new.tolist())
        components.append(queue)
        if min_size <= len(queue) <= max_size:
            clusters.append(queue)
    clusters.sort(key=lambda c: -len(c))  # list.sort is stable: THIS PROJECT'S READING of the std::sort
    return clusters, components


def _points(x, y, z, indices):
    pts = np.stack([np.asarray(v, dtype=F) for v in (x, y, z)], axis=1)
    if indices is None:
        return pts, np.arange(pts.shape[0], dtype=np.uint32)
    indices = np.asarray(indices, dtype=np.uint32)
    return pts[indices.astype(np.int64)], indices  # PointCloud::extract


def csr(clusters, entries):
    sizes = [len(c) for c in clusters]
    flat = np.asarray([p for c in clusters for p in c], dtype=np.int64)
    return entries[flat].astype(np.uint32), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


def euclidean_cluster(x, y, z, tolerance=0.5, min_size=10, max_size=100000, indices=None):
    """euclideanCluster(cloud[, subset_indices], config): (indices, offsets) in the reference's BFS order, the positions
    remapped to the list's entries; also the clusters as lists of POSITIONS."""
    pts, entries = _points(x, y, z, indices)
    clusters, _ = cluster_core(pts, tolerance, min_size, max_size)
    ind, off = csr(clusters, entries)
    return ind, off, clusters


def canonical(clusters, entries, m):
    """What the device returns: clusters (lists of positions) in descending size, equal sizes by smallest position;
    inside a cluster ascending position.  (indices, offsets, labels per position)."""
    ordered = sorted((sorted(c) for c in clusters), key=lambda c: (-len(c), c[0]))
    ind, off = csr(ordered, entries)
    labels = np.zeros(m, dtype=np.uint32)
    for k, c in enumerate(ordered):
        labels[np.asarray(c, dtype=np.int64)] = k + 1
    return ind, off, labels


def noise_indices(indices, total):
    mask = np.ones(total, dtype=bool)
    mask[indices.astype(np.int64)] = False
    return np.nonzero(mask)[0].astype(np.uint32)


def apply_cluster_labels(indices, offsets, total, semantic_class=0):
    out = np.full(total, (semantic_class & 0xFFFF) << 16, dtype=np.uint32)
    for k in range(offsets.size - 1):
        out[indices[offsets[k]:offsets[k + 1]].astype(np.int64)] = ((semantic_class & 0xFFFF) << 16) | ((k + 1) & 0xFFFF)
    return out


# ---- the relation alone: near pairs, brute-force components, the admission check ----
def near_pairs(pts, tolerance, slab):
    """Blocks (i, j, d64) of all pairs i < j whose voxel x coordinates differ by at most `slab`, with their squared
    distance in float64.  Pruning by x alone is exact for slab >= range: the relation asks it of every axis."""
    inv, _, _ = relation_constants(tolerance)
    vx = voxels(pts, inv)[:, 0]
    order = np.argsort(vx, kind="stable")
    svx, p64 = vx[order], pts[order].astype(np.float64)
    m = pts.shape[0]
    step = 512
    for a in range(0, m, step):
        b = min(a + step, m)
        hi = int(np.searchsorted(svx, svx[b - 1] + slab, side="right"))
        if hi <= a + 1:
            continue
        d = p64[a:b, None, :] - p64[None, a:hi, :]
        d64 = (d * d).sum(axis=2)
        ii, jj = np.nonzero((np.arange(a, b)[:, None] < np.arange(a, hi)[None, :]) &
                            (svx[None, a:hi] - svx[a:b, None] <= slab))
        yield order[a + ii], order[a + jj], d64[ii, jj]


def components_brute(x, y, z, tolerance, indices=None):
    """The connected components of the relation over the list positions, by testing every pair (pruned by the voxel x
    condition, which is part of the relation): label[p] = the component's smallest position."""
    pts, _ = _points(x, y, z, indices)
    m = pts.shape[0]
    inv, r_sq, rng = relation_constants(tolerance)
    vox = voxels(pts, inv)
    edges_i, edges_j = [], []
    for i, j, _ in near_pairs(pts, tolerance, rng):
        ok = (np.abs(vox[i] - vox[j]) <= rng).all(axis=1) & (dist_sq(pts[i], pts[j]) <= r_sq)
        edges_i.append(i[ok])
        edges_j.append(j[ok])
    label = np.arange(m, dtype=np.int64)
    if edges_i:
        ei, ej = np.concatenate(edges_i), np.concatenate(edges_j)
        while True:  # minimum-label propagation with pointer jumping, to the fixed point
            low = np.minimum(label[ei], label[ej])
            new = label.copy()
            np.minimum.at(new, ei, low)
            np.minimum.at(new, ej, low)
            new = new[new]
            if np.array_equal(new, label):
                break
            label = new
    return label


def clusters_of_labels(label, min_size, max_size):
    """The kept components of a labelling as lists of positions (in no particular order)."""
    order = np.argsort(label, kind="stable")
    cuts = np.nonzero(np.diff(label[order]))[0] + 1
    return [c.tolist() for c in np.split(order, cuts) if min_size <= c.size <= max_size] if label.size else []


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in float64; the sum is rounded to double, then to
    float (a double rounding could differ from a true fma in about one case in 2^29: enough for an admission check)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def decisions(a, b, r_sq):
    """dist_sq <= r_sq under the three fp32 summation orders and two fused forms: [5, k] booleans."""
    d = (a - b).astype(F)
    s0, s1, s2 = (d[:, k] * d[:, k] for k in range(3))
    forms = [s0 + (s1 + s2), (s0 + s1) + s2, (s0 + s2) + s1,
             _fma(d[:, 2], d[:, 2], _fma(d[:, 1], d[:, 1], s0)), _fma(d[:, 0], d[:, 0], _fma(d[:, 1], d[:, 1], s2))]
    return np.stack([f <= r_sq for f in forms])


def admission(x, y, z, tolerance, indices=None, cap=1e-5):
    """(pairs inside the band r_sq (1 +- cap) in float64, those of them whose decision depends on the fp32 summation
    order or on fusing).  A case is admitted iff the second number is 0."""
    pts, _ = _points(x, y, z, indices)
    _, r_sq, rng = relation_constants(tolerance)
    band = undecided = 0
    for i, j, d64 in near_pairs(pts, tolerance, rng + 1):
        close = np.abs(d64 - float(r_sq)) <= cap * float(r_sq)
        if close.any():
            dec = decisions(pts[i[close]], pts[j[close]], r_sq)
            band += int(close.sum())
            undecided += int((dec != dec[0]).any(axis=0).sum())
    return band, undecided
