"""tests/voxel_restate.py — the NumPy restatement the GPU downsampling filters are held against — checked on its own:
the reference's known answers (nanoPCL tests/test_filters.cpp:159-317 and the empty, single-point and NaN cases at
:786-812), its ANY mode against the oracle's voxelGrid(ANY) in both orders, its key against the oracle's voxel::pack."""
import numpy as np
import pytest

import voxel_restate as V
from voxel_restate import M      # scripts/introsort_model

F32 = np.float32


def cloud(points):
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


# ---- test_filters.cpp:159-317 ----
def test_voxelGrid_centroid():
    r = V.voxel_grid(*cloud([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]), 2.0, "centroid")
    assert r["x"].size == 1
    assert (r["x"][0], r["y"][0], r["z"][0]) == (F32(0.5), F32(0.5), F32(0.0))


def test_voxelGrid_nearest():
    r = V.voxel_grid(*cloud([(0.1, 0.1, 0), (0.9, 0.1, 0), (0.1, 0.9, 0), (0.5, 0.5, 0)]), 1.0, "nearest")
    assert r["x"].size == 1 and r["idx"][0] == 3
    assert (r["x"][0], r["y"][0]) == (F32(0.5), F32(0.5))


def test_voxelGrid_channel_averaging():
    r = V.voxel_grid(*cloud([(0, 0, 0), (0.5, 0.5, 0)]), 1.0, "centroid", intensity=[0.2, 0.8])
    assert r["x"].size == 1 and r["intensity"] is not None
    assert abs(float(r["intensity"][0]) - 0.5) < 0.01
    assert r["intensity"][0] == (F32(0) + F32(0.2) + F32(0.8)) / F32(2)


def test_voxelGrid_move_semantics_grid3x3x3():
    g = [(x, y, z) for x in range(3) for y in range(3) for z in range(3)]
    r = V.voxel_grid(*cloud(g), 1.5)
    assert 0 < r["x"].size < 27 and r["x"].size == 8


def test_voxelGrid_covariance_preservation():
    cov = np.stack([np.eye(3, dtype=F32).reshape(9) * 2, np.eye(3, dtype=F32).reshape(9) * 4])
    r = V.voxel_grid(*cloud([(0, 0, 0), (0.5, 0.5, 0)]), 1.0, "centroid", cov=cov)
    assert r["x"].size == 1 and r["cov9"][0, 0] == 2.0 and r["idx"][0] == 0      # the representative's


def test_voxelGrid_symmetry():
    pts, x = [], F32(-10.0)
    while x <= F32(10.0):
        y = F32(-10.0)
        while y <= F32(10.0):
            pts.append((x, y, 0.0))
            y = F32(y + F32(0.3))
        x = F32(x + F32(0.3))
    cx, cy, cz = cloud(pts)
    r = V.voxel_grid(cx, cy, cz, 0.3)
    orig, down = float((cx < 0).sum()) / cx.size, float((r["x"] < 0).sum()) / r["x"].size
    assert abs(orig - down) < 0.05 and 0.45 < down < 0.55


def test_gridMaxZ_basic():
    r = V.grid_max_z(*cloud([(0, 0, 1), (0, 0, 5), (0, 0, 3)]), 1.0)
    assert r["z"].tolist() == [5.0]


def test_gridMaxZ_multiple_cells():
    r = V.grid_max_z(*cloud([(0, 0, 1), (0, 0, 3), (2, 0, 5), (2, 0, 2)]), 1.0)
    assert r["z"].tolist() == [3.0, 5.0] and r["idx"].tolist() == [1, 2]


def test_gridMaxZ_channel_preservation():
    r = V.grid_max_z(*cloud([(0, 0, 1), (0, 0, 5)]), 1.0, intensity=[0.1, 0.9])
    assert r["x"].size == 1 and r["intensity"][0] == F32(0.9)


# ---- test_filters.cpp:786-812 ----
def test_empty_single_point_and_nan():
    e = np.zeros(0, dtype=F32)
    assert V.voxel_grid(e, e, e, 1.0)["x"].size == 0 and V.grid_max_z(e, e, e, 1.0)["x"].size == 0
    one = cloud([(1, 2, 3)])
    assert V.voxel_grid(*one, 1.0)["x"].size == 1 and V.grid_max_z(*one, 1.0)["x"].size == 1
    r = V.voxel_grid(*cloud([(1, 2, 3), (np.nan, 0, 0), (4, 5, 6)]), 10.0)
    assert r["x"].size == 1 and (r["x"][0], r["y"][0], r["z"][0]) == (F32(2.5), F32(3.5), F32(4.5))


def test_size_limits():
    one = cloud([(1, 2, 3)])
    for ok in (0.001, 100.0):
        assert V.voxel_grid(*one, ok)["x"].size == 1 and V.grid_max_z(*one, ok)["x"].size == 1
    for bad in (0.0009, 100.5, float("nan")):
        with pytest.raises(ValueError, match=r"voxel_size must be in \[0.001, 100\]"):
            V.voxel_grid(*one, bad)
        with pytest.raises(ValueError, match=r"grid_size must be in \[0.001, 100\]"):
            V.grid_max_z(*one, bad)


# ---- ANY against the oracle's voxelGrid(ANY), both orders ----
def tied(rng, n, cells):
    c = rng.integers(0, cells, n)
    x = (c % 7) * 0.25 + rng.uniform(0.01, 0.24, n) - 1.0
    y = ((c // 7) % 7) * 0.25 + rng.uniform(0.01, 0.24, n) - 1.0
    z = (c // 49) * 0.25 + rng.uniform(0.01, 0.24, n)
    return x.astype(F32), y.astype(F32), z.astype(F32)


def any_clouds():
    rng = np.random.default_rng(11)
    yield "random", tuple(rng.uniform(-20, 20, 3000).astype(F32) for _ in range(3))
    yield "tie_heavy", tied(rng, 3000, 40)
    x, y, z = tied(rng, 2000, 60)
    x[::17] = np.nan
    z[5::31] = np.inf
    yield "non_finite", (x, y, z)
    k = np.asarray(M.median3_killer(2000), dtype=np.float64)
    yield "median3_killer", ((k * 0.25 + 0.125).astype(F32) - F32(300.0), rng.uniform(0.01, 0.24, 2000).astype(F32),
                             np.full(2000, 0.1, dtype=F32))


@pytest.mark.parametrize("name,xyz", list(any_clouds()), ids=[n for n, _ in any_clouds()])
def test_any_equals_the_oracle(R, name, xyz):
    picks = {}
    for order in (0, 1):
        want = R.voxel_any(*xyz, 0.25, stable=order == 0)
        got = V.voxel_grid(*xyz, 0.25, "any", order=order)
        assert np.array_equal(got["idx"], want), (name, order)
        assert np.array_equal(got["x"], xyz[0][want])
        picks[order] = want
    if name != "random":
        assert not np.array_equal(picks[0], picks[1]), "input without teeth: both orders pick the same points"


# ---- the key against the oracle's voxel::pack ----
@pytest.mark.parametrize("size", [0.001, 0.05, 0.25, 100.0])
def test_key_equals_the_oracle(R, size):
    inv = F32(1.0) / F32(size)
    edge = F32(1 << 20) * F32(size)
    vals = [0.0, -0.0, 0.1, -0.1, -1e-30, 1e-30, 3.75, -3.75, -size, size, float(edge), float(-edge),
            float(np.nextafter(edge, F32(0))), float(np.nextafter(-edge, F32(0))), float(edge * F32(2)), float(-edge * F32(2)),
            2.2e9 * size, -2.2e9 * size, 1e30, -1e30, 3.0e38, -3.0e38]
    rng = np.random.default_rng(3)
    pts = np.asarray([(rng.choice(vals), rng.choice(vals), rng.choice(vals)) for _ in range(400)] +
                     [(v, v, v) for v in vals], dtype=F32)
    valid, key = V.keys_of(pts[:, 0], pts[:, 1], pts[:, 2], size)
    flat_valid, flat = V.keys_of(pts[:, 0], pts[:, 1], pts[:, 2], size, flat=True)
    assert valid.all() and flat_valid.all()
    ix, iy, iz = V.unpack(key)
    for i, p in enumerate(pts):
        want, fields = R.voxel_pack(p[0], p[1], p[2], inv)
        assert int(key[i]) == want, (p, hex(int(key[i])), hex(want))
        assert (int(ix[i]), int(iy[i]), int(iz[i])) == fields
        assert int(flat[i]) == R.voxel_pack(p[0], p[1], 0.0, inv)[0]
    assert (np.abs(ix) >= (1 << 20) - 1).any() and (ix < 0).any()      # the clamp and negative indices were reached
