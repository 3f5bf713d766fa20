"""Compact winner slots of the batch pipeline (fastdem_amd/csrc/fdm_multi.hpp, mbin_body's merge).  A bin block leaves
its block-local minimum's {z, sigma_z^2} and its block-local last point's colour at the block's SLOT for the cell —
lb * 512 + the cell's rank in the block's compacted table — and the reduced key (low word) and aux.w carry that slot
instead of a point index.  Across the bin blocks of one scan the order must stay the reference's: on equal heights the
first point wins (strict "<", elevation_mapping.cpp:41-92), the colour is the last point's.  Checked against the CPU
oracle run scan by scan, through batch launches (check_batch asserts that batch launches were taken).

Run on the GPU box:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from helpers import pair
from test_batch_gpu import T, check_batch, cloud

pytestmark = pytest.mark.gpu
F32 = np.float32


def _local(c):
    c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 3.0, 0.0, 30.0


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_equal_minimum_in_several_bin_blocks_the_first_point_wins(gpu, R, estimation_type):
    """One cell, one height, in bin blocks 0, 1 and 3 of the same scan (points 7, 700, 1600 at different sensor-frame
    positions, so their sigma_z^2 differ): the map must take the observation of point 7.  Colour: the last of them."""
    def fill(c):
        _local(c)
        c.estimation_type = estimation_type

    eng, ref = pair(gpu, R, 8.0, 8.0, 0.1, fill)
    rng = np.random.default_rng(101)
    scans, poses = [], []
    for k in range(7):
        s = cloud(rng, 2000 + 301 * k, 3.5, intensity=True, rgb=True)
        for i, dx in ((7, 0.0), (700, 0.02), (1600, 0.04)):  # (whole-cell poses: the three stay in one cell, 0.03 m from its edges)
            s["x"][i], s["y"][i], s["z"][i] = F32(1.03 + dx), F32(-0.55), F32(-0.75)
        scans.append(s)
        poses.append(T(0.1 * k, 0.0, 0.0))
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), poses)


def test_signed_zero_minima_and_maxima_across_bin_blocks(gpu, R):
    """+-0 heights and intensities, a few distinct heights only (ties everywhere) and NaN intensities, 1 700 points per
    scan on a 64-cell map: every cell is hit by every bin block of every scan."""
    def fill(c):
        c.mode = 1
        c.sensor_type = 0

    eng, ref = pair(gpu, R, 4.0, 4.0, 0.5, fill)
    rng = np.random.default_rng(3)
    scans = []
    for k in range(11):
        n = 1700
        x = rng.uniform(-1.9, 1.9, n).astype(F32)
        y = rng.uniform(-1.9, 1.9, n).astype(F32)
        z = rng.choice(np.array([0.0, -0.0, 0.25, -0.25, 0.5], dtype=F32), n)
        a = rng.choice(np.array([0.0, -0.0, np.nan, 0.5, 0.75], dtype=F32), n)
        rgb = rng.integers(0, 1 << 24, n, dtype=np.uint32)
        scans.append({"x": x, "y": y, "z": z, "intensity": a, "rgb": rgb})
    check_batch(gpu, R, eng, ref, scans, T(), [T() for _ in range(11)])


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_dense_blocks_probe_collisions_and_ragged_scan_sizes(gpu, R, estimation_type):
    """Points spread over a 14 400-cell map: a 512-point bin block touches ~500 cells, so its LDS table (cell mod 512)
    is full of probe chains and the slots of its compacted list run up to ~500.  Scan sizes that are not multiples of
    512 (a last block with 1, 511 or 513 points; scans of one point and of 511)."""
    def fill(c):
        _local(c)
        c.estimation_type = estimation_type

    eng, ref = pair(gpu, R, 12.0, 12.0, 0.1, fill)
    rng = np.random.default_rng(17)
    sizes = [5121, 511, 4607, 1, 2049, 3583, 513, 5000, 1024, 4097, 2560, 777, 5119, 3, 4608, 1537, 2047, 4096]
    scans, poses = [], []
    for k, n in enumerate(sizes):
        scans.append(cloud(rng, n, 5.9, intensity=True, rgb=True))
        poses.append(T(0.07 * k, -0.04 * k, 0.0, yaw=0.02 * k))
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), poses)


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_sixteen_scans_on_the_same_cells(gpu, R, estimation_type):
    """16 scans in one launch, each of 3 000 points in the same nine cells, heights from a small set: every event of
    the update holds a winner from another bin block of another scan."""
    def fill(c):
        _local(c)
        c.estimation_type = estimation_type

    eng, ref = pair(gpu, R, 6.0, 6.0, 0.1, fill)
    eng.set_option("batch_max", 16)
    rng = np.random.default_rng(23)
    scans = []
    for k in range(17):
        n = 3000
        s = {"x": rng.uniform(0.4, 0.69, n).astype(F32), "y": rng.uniform(-0.29, 0.0, n).astype(F32),
             "z": rng.choice(np.array([-0.3, -0.1, 0.0, 0.2, 0.45], dtype=F32), n),
             "intensity": rng.uniform(0, 1, n).astype(F32), "rgb": rng.integers(0, 1 << 24, n, dtype=np.uint32)}
        scans.append(s)
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), [T() for _ in range(17)])


@pytest.mark.parametrize("batch_walk", [0, 1])
def test_walker_off_and_on_with_a_filtered_scan_and_a_jump_beyond_the_map(gpu, R, batch_walk):
    """LOCAL mode (the move of a scan is gated on a surviving point).  Scans 5, 6 and 21 have none, so they do not move
    the map: the walker's chain (it assumes every scan passes) is wrong behind them and the bin blocks walk
    themselves.  Scan 15 jumps beyond the map (everything cleared), scan 16 comes back.  Colour on the first call."""
    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -1.0, 2.0, 0.5, 20.0

    eng, ref = pair(gpu, R, 10.0, 8.0, 0.1, fill)
    eng.set_option("batch_walk", batch_walk)
    rng = np.random.default_rng(61)
    scans, poses = [], []
    for k in range(34):
        s = cloud(rng, 2500 + 97 * k, 3.8, intensity=True, rgb=k < 10)
        if k in (5, 6, 21):
            s["z"] = (s["z"] + 40.0).astype(F32)
        scans.append(s)
        px = 30.0 if k == 15 else 0.23 * k
        poses.append(T(px, 0.11 * k * (-1) ** k, 0.0, yaw=0.04 * k))
    check_batch(gpu, R, eng, ref, scans[:10], T(z=0.4), poses[:10])
    check_batch(gpu, R, eng, ref, scans[10:], T(z=0.4), poses[10:])
    check_batch(gpu, R, eng, ref, scans[10:30], T(z=0.4), [T(-0.13 * k, 0.2, 0.0) for k in range(20)])


def test_image_ordered_quantile_colour_intensity(gpu, R):
    """configs[2]'s setting — P2 estimator, RGB-D sensor model, colour and intensity — on image-ordered clouds whose
    neighbouring points fall into the same cell in runs (the wavefront run merge ahead of the LDS table): the colour
    of a cell is its last point's across the bin blocks."""
    def fill(c):
        c.mode = 1
        c.estimation_type = 1
        c.sensor_type = 2
        c.z_min, c.z_max = -5.0, 5.0

    eng, ref = pair(gpu, R, 6.0, 6.0, 0.05, fill)
    rng = np.random.default_rng(29)
    h, w = 40, 400
    scans = []
    for k in range(20):
        u, v = np.meshgrid(np.linspace(-2.5, 2.5, w), np.linspace(-2.0, 2.0, h))
        x = (u + 0.01 * k).astype(F32).ravel()
        y = (v - 0.02 * k).astype(F32).ravel()
        z = (1.0 + 0.1 * np.round(rng.standard_normal(h * w) * 3)).astype(F32)
        scans.append({"x": x, "y": y, "z": z, "intensity": rng.uniform(0, 1, h * w).astype(F32),
                      "rgb": rng.integers(0, 1 << 24, h * w, dtype=np.uint32)})
    check_batch(gpu, R, eng, ref, scans, T(z=0.1), [T(0.01 * k, 0.0, 0.0) for k in range(20)])
