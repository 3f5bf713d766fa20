"""The update half of the batch pipeline (fastdem_amd/csrc/fdm_multi.hpp, mupdate_body) with one wavefront owning the
block's cells: thread (group q, cell c) = q * cells_per_block + c looks after scans 4 q .. 4 q + 3 of cell c, the cell
masks travel through LDS, and the owners — the first cells_per_block threads — apply the events.  What can go wrong
with that mapping: a partial last block (cells missing in the middle of the owner wavefront), the switch from four to
eight threads per cell beyond 16 scans, groups without a scan, a cell whose events straddle the two exchange rounds,
owners with 16 events beside owners with none, blocks without events, strips vacated between a cell's events, the
colour hand-over and the ray events.  Every case against the CPU oracle run scan by scan, through batch launches.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from helpers import pair
from test_batch_gpu import T, check_batch, cloud
from test_batch_ray_gpu import batch_vs_oracle, ray_on

pytestmark = pytest.mark.gpu
F32 = np.float32


def _open(c):
    c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 3.0, 0.0, 30.0


def _fill(estimation_type=0, mode=0):
    def fill(c):
        _open(c)
        c.estimation_type = estimation_type
        c.mode = mode
    return fill


# (cells, scans per launch): 63 and 35 cells are one partial block of 64 (29 owners missing in the middle of the owner
# wavefront) and two blocks of 32 with a partial second one; 150 x 150 = 22 500 cells ends in a block of 36 / of 4 cells
@pytest.mark.parametrize("batch_max", [16, 32])
@pytest.mark.parametrize("cells", [(9, 7), (5, 7), (150, 150)])
def test_partial_last_block(gpu, R, cells, batch_max):
    res = 0.5 if cells[0] < 100 else 0.1
    w, h = cells[0] * res, cells[1] * res
    eng, ref = pair(gpu, R, w, h, res, _fill(mode=1))
    assert eng.geometry().rows * eng.geometry().cols == cells[0] * cells[1]
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(cells[0] * 100 + batch_max)
    n_scans = 1 + batch_max + 3
    scans = []
    for k in range(n_scans):
        s = cloud(rng, 3000, 0.5 * max(w, h), intensity=True)
        # the last cells in memory order are map corners: some points in every corner cell
        for i, (sx, sy) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
            s["x"][i::500] = F32(sx * (0.5 * w - 0.3 * res))
            s["y"][i::500] = F32(sy * (0.5 * h - 0.3 * res))
        scans.append(s)
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), [T() for _ in range(n_scans)])


@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [2, 3, 4, 5, 15, 16, 17, 32])
def test_scans_per_launch(gpu, R, batch_max, estimation_type):
    """41 scans: one alone (it creates the layers), then launches of batch_max scans and a shorter last one — 2 ... 16
    scans take four threads per cell (groups beyond the count hold no scan), 17 and 32 take eight.  LOCAL map, a shift
    every scan, 77 x 59 cells (no multiple of 64 or 32)."""
    eng, ref = pair(gpu, R, 7.7, 5.9, 0.1, _fill(estimation_type))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(1000 + batch_max)
    scans, poses = [], []
    for k in range(41):
        scans.append(cloud(rng, 1200 + 31 * k, 4.0, intensity=True))
        poses.append(T(0.13 * k, -0.07 * k * (-1) ** (k // 3), 0.0, yaw=0.05 * k))
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), poses)


def _every_cell(rng, short_cell, short, k):
    """Three points in every cell of a 4 x 4 m map at 0.5 m; in scan k of the `short` set none in `short_cell`."""
    c = (np.arange(8) - 3.5) * 0.5
    x, y = np.meshgrid(c, c, indexing="ij")
    x, y = np.repeat(x.ravel(), 3), np.repeat(y.ravel(), 3)
    if k in short and short_cell is not None:
        keep = ~((np.sign(x) == short_cell[0]) & (np.abs(x) > 1.5) & (np.sign(y) == short_cell[1]) & (np.abs(y) > 1.5))
        x, y = x[keep], y[keep]
    n = x.size
    return {"x": (x + rng.uniform(-0.2, 0.2, n)).astype(F32), "y": (y + rng.uniform(-0.2, 0.2, n)).astype(F32),
            "z": rng.choice(np.array([-0.3, -0.1, 0.0, 0.2, 0.45], dtype=F32), n),
            "intensity": rng.uniform(0, 1, n).astype(F32), "rgb": rng.integers(0, 1 << 24, n, dtype=np.uint32)}


@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [16, 32])
@pytest.mark.parametrize("short_cell", [None, (1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_two_exchange_rounds(gpu, R, short_cell, batch_max, estimation_type):
    """An 8 x 8-cell map hit in every cell by every scan of a launch: 1 024 events per block (64 cells x 16 scans, or
    32 cells x 32 scans), two rounds of the exchange, event 512 the first of a cell.  With one corner cell left out of
    half the launch's scans — whichever corner is the first cell in memory order — event 512 falls inside a cell: its
    owner stops in the middle of its events and goes on in round two."""
    eng, ref = pair(gpu, R, 4.0, 4.0, 0.5, _fill(estimation_type, mode=1))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(7 + batch_max)
    n_scans = 1 + batch_max
    short = set(range(1 + batch_max // 2, n_scans))
    scans = [_every_cell(rng, short_cell, short, k) for k in range(n_scans)]
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), [T() for _ in range(n_scans)])


@pytest.mark.parametrize("batch_max", [16, 32])
def test_sparse_and_dense_owners_side_by_side_and_empty_blocks(gpu, R, batch_max):
    """Every scan puts 2 000 points into the same 27 cells — every third cell of a line along x, of a line along y and
    of a diagonal, so an owner with an event in every scan sits between owners with none — and 40 points anywhere on
    the 120 x 120-cell map: most update blocks see no event at all, some see a single one."""
    eng, ref = pair(gpu, R, 12.0, 12.0, 0.1, _fill(mode=1))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(55)
    j = 3 * np.arange(9)
    cx = np.concatenate([0.05 + 0.1 * j, np.full(9, 2.05), -3.05 + 0.1 * j])
    cy = np.concatenate([np.full(9, -1.05), 0.05 + 0.1 * j, 3.05 - 0.1 * j])
    n_scans = 1 + batch_max + 2
    scans = []
    for k in range(n_scans):
        pick = rng.integers(0, cx.size, 2000)
        s = cloud(rng, 2040, 5.9, intensity=True)
        s["x"][:2000] = (cx[pick] + rng.uniform(-0.04, 0.04, 2000)).astype(F32)
        s["y"][:2000] = (cy[pick] + rng.uniform(-0.04, 0.04, 2000)).astype(F32)
        scans.append(s)
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), [T() for _ in range(n_scans)])


@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [16, 32])
def test_moves_between_a_cells_events(gpu, R, batch_max, estimation_type):
    """LOCAL mode: strips vacated between the events of a cell (wiped by its owner between two estimator steps), scans
    5, 6 and 21 without a surviving point (they do not move the map), a jump beyond the map at scan 15 and back.
    Colour in the first call."""
    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -1.0, 2.0, 0.5, 20.0
        c.estimation_type = estimation_type

    eng, ref = pair(gpu, R, 9.7, 7.9, 0.1, fill)
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(61 + batch_max)
    scans, poses = [], []
    for k in range(36):
        s = cloud(rng, 2500 + 97 * k, 3.8, intensity=True, rgb=k < 18)
        if k in (5, 6, 21):
            s["z"] = (s["z"] + 40.0).astype(F32)
        scans.append(s)
        px = 30.0 if k == 15 else 0.23 * k
        poses.append(T(px, 0.11 * k * (-1) ** k, 0.0, yaw=0.04 * k))
    check_batch(gpu, R, eng, ref, scans[:18], T(z=0.4), poses[:18])
    check_batch(gpu, R, eng, ref, scans[18:], T(z=0.4), poses[18:])


@pytest.mark.parametrize("batch_max", [16, 32])
def test_colour_of_the_last_event(gpu, R, batch_max):
    """Colour + intensity on dense cells: the owner takes each event's colour from the exchange, the cell keeps the
    last one's.  63 cells, every one hit by most scans."""
    eng, ref = pair(gpu, R, 4.5, 3.5, 0.5, _fill(mode=1))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(88)
    n_scans = 1 + batch_max + 1
    scans = [cloud(rng, 150 + 7 * k, 2.4, intensity=True, rgb=True) for k in range(n_scans)]
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), [T(0.0, 0.0, 0.0, yaw=0.1 * k) for k in range(n_scans)])


@pytest.mark.parametrize("batch_max", [5, 16, 32])
def test_ray_events_with_and_without_observations(gpu, R, batch_max):
    """raycast_enabled: the owners fetch their records with the first round trip and resolve every scan's ray events
    behind that scan's observation; most cells a ray crosses hold no observation of that scan.  Aggressive ghost
    removal, LOCAL shifts, a jump beyond the map; 77 x 59 cells."""
    eng, ref = pair(gpu, R, 7.7, 5.9, 0.1, ray_on(_open, rc_log_odds_ghost=0.9, rc_clear_threshold=-0.5,
                                                   rc_height_conflict_threshold=0.02))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(5)
    steps = [(0, 0), (0.35, 0), (0.35, -0.4), (-1.2, 0.9), (-1.2, 0.9), (3.1, 3.3), (40.0, -25.0), (40.1, -25.0),
             (0.0, 0.0), (0.05, 0.04)] + [(0.1 * k, -0.05 * k) for k in range(1, 28)]
    scans, poses = [], []
    for k, (px, py) in enumerate(steps):
        n = int(rng.integers(200, 3000))
        s = cloud(rng, n, 4.5, intensity=True, rgb=k % 2 == 0 and k < 12)
        s["z"] = (s["z"] + F32(0.6) * (rng.uniform(size=n) < 0.3)).astype(F32)  # bumps that later rays pass through
        scans.append(s)
        poses.append(T(px, py, 0.0, yaw=0.1 * k))
    cleared = batch_vs_oracle(gpu, eng, ref, scans, T(z=1.5), poses)
    assert cleared > 0


@pytest.mark.parametrize("extra", [3, 60])
@pytest.mark.parametrize("batch_max", [16, 32])
def test_ray_wipe_of_every_layer(gpu, R, batch_max, extra):
    """raycast_enabled with plain layers added before the first scan: the owners' all-layer wipe (a vacated strip, or a
    ghost cell's clearAt) fetches its pointers in groups of eight, the last group clamped to the last layer — with 3 added
    layers the layer count is no multiple of eight, with 60 it is beyond 64.  12 x 9 = 108 cells: the last update block
    is partial at 64 and at 32 cells per block.  One-cell LOCAL shifts in front of some scans, the batch's last one
    among them.  Every layer, the added ones included, against the oracle."""
    eng, ref = pair(gpu, R, 1.2, 0.9, 0.1, ray_on(_open, rc_log_odds_ghost=0.9, rc_clear_threshold=-0.5,
                                                   rc_height_conflict_threshold=0.02))
    assert eng.geometry().rows * eng.geometry().cols == 108
    eng.set_option("batch_max", batch_max)
    for o in (eng, ref):
        for i in range(extra):
            o.add("extra_%02d" % i, 1.0 + i)
    rng = np.random.default_rng(300 + batch_max + extra)
    scans, poses = [], []
    px = 0.0
    for k in range(32):
        n = int(rng.integers(100, 301))
        s = cloud(rng, n, 0.7, intensity=True)
        s["x"] = np.abs(s["x"])  # points and rays ahead of the robot only: the cells behind it keep what they hold
        s["z"] = (s["z"] + F32(0.6) * (rng.uniform(size=n) < 0.3)).astype(F32)  # bumps that later rays pass through
        scans.append(s)
        # the first scan goes alone (it creates the estimator's layers), then launches of batch_max: a shift in front
        # of scans 5 and 11, and of the last scan of every launch (16, 31 | 31)
        if k in (5, 11, 16, 31):
            px += 0.1
        poses.append(T(px, 0.0, 0.0))
    cleared = batch_vs_oracle(gpu, eng, ref, scans, T(z=1.5), poses)
    assert cleared > 0
    last = eng.layer("extra_%02d" % (extra - 1))
    assert np.isnan(last).any() and (last == F32(extra)).any()
