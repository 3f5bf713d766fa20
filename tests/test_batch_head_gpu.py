"""k_mbatch's arguments (fastdem_amd/csrc/fdm_multi.hpp): a head of leading scalars that dispatches every block, one
record per scan (MBinScan / MCropScan) indexed by the block's row, a `prev` state that is always readable with a flag
beside it, the update half's key and state pointers among the leading arguments.  What can go wrong there is indexing:
scan k's n or pointers taken from another record, the grid's width, the select between "the previous batch's state"
and "the geometry ring" — so every call here mixes scan sizes inside a batch (1 ... 1 500 points: one to three bin
blocks, the widest scan sets the grid and the short rows' surplus blocks leave), moves the LOCAL map on most scans,
holds scans whose points are all cropped (they must not move the map) and goes out as two calls, each long enough
for a first batch (scouts in a launch of their own, no `prev`), fused batches, and a last update flushed alone.

Each call is compared with the CPU oracle run scan by scan (NaN pattern, rtol 1e-5, statistics, geometry; the cell ids
through the engine that integrates the same scans one by one) and with that engine (every layer exactly).

Run on the GPU box:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from helpers import assert_arrays_close, assert_layers_equal, pair, run_both, same_geometry
from test_batch_gpu import DeviceBatch, T, cloud

pytestmark = pytest.mark.gpu
F32 = np.float32

SIZES = [1, 3, 511, 512, 513, 1024, 1500]   # below / at / above one and two 512-point bin blocks
N_SCANS = 41                                 # 1 (creates the layers) + 40: 2 x 16 + 8, 17 + 17 + 6, 32 + 8, twenty pairs
CROPPED = (6, 19, 33)                        # scans whose points all fail cropZ


def crops(c):
    c.z_min, c.z_max, c.range_min, c.range_max = -1.0, 2.0, 0.2, 20.0


def stream(seed, intensity, rgb):
    """N_SCANS ragged scans on a 40 x 40 cell LOCAL map and poses that move it on most of them."""
    rng = np.random.default_rng(seed)
    scans, poses = [], []
    for k in range(N_SCANS):
        n = SIZES[(k * 3 + k // 7) % len(SIZES)]
        s = cloud(rng, n, 1.9, intensity=intensity, rgb=rgb)
        if k in CROPPED:
            s["z"] = (s["z"] + 50.0).astype(F32)
        scans.append(s)
        poses.append(T(0.13 * k, -0.07 * k + 0.3 * np.sin(0.5 * k), 0.0, yaw=0.04 * k))
    return scans, poses


def one_by_one(eng, ref, scans, Tbs, poses):
    """The oracle and an engine without batch launches, scan by scan; cell ids and statistics checked at every scan."""
    last = None
    for s, Twb in zip(scans, poses):
        last = run_both(eng, ref, s, Tbs, Twb)
    return last


def check_call(gpu, R, fill, scans, poses, batch_max, Tbs=None):
    Tbs = T(z=0.4) if Tbs is None else Tbs
    single, ref = pair(gpu, R, 4.0, 4.0, 0.1, fill)
    single.set_option("batch", 0)
    last = one_by_one(single, ref, scans, Tbs, poses)
    eng, _ = pair(gpu, R, 4.0, 4.0, 0.1, fill)
    eng.enable_cell_ids(False)  # (an engine that owes its caller cell ids takes no batch launch)
    eng.set_option("batch_max", batch_max)
    # two calls with a sync between them: the held-back update of the first call's last batch is flushed alone, and the
    # second call's first batch has no `prev` on a map that has moved (the geometry ring and the batch's own, zeroed
    # state then differ: the select between them shows)
    cut = min(23, len(scans) - 3)
    b = DeviceBatch(gpu, scans[:cut], Tbs, poses[:cut])
    assert eng.integrate_device_batch(b.arr) == 0
    eng.sync()
    b2 = DeviceBatch(gpu, scans[cut:], Tbs, poses[cut:])
    assert eng.integrate_device_batch(b2.arr) == 0
    # (the `tiled_all` variant of the fixture pushes every scan through the record pools, one fused launch per scan: the
    # same comparisons then cover that path)
    if "tiled_min" not in gpu.Engine.default_options:
        assert sum(eng.batch_launches()) >= (len(scans) - 2) // batch_max, "the calls took too few batch launches"
    assert eng.last_stats() == last
    assert_layers_equal(eng, ref)
    assert same_geometry(eng.geometry(), ref.geometry())
    for name in single.layers():
        assert_arrays_close(eng.layer(name), single.layer(name), name, 0.0, 0.0)
    return eng


@pytest.mark.parametrize("batch_max", [2, 3, 16])
@pytest.mark.parametrize("channels", ["none", "intensity", "colour", "both"])
def test_kalman_ragged_batches(gpu, R, channels, batch_max):
    """Every channel set (one k_mbatch instantiation each) at batch sizes 2, 3 and 16."""
    scans, poses = stream(7, channels in ("intensity", "both"), channels in ("colour", "both"))
    eng = check_call(gpu, R, crops, scans, poses, batch_max)
    assert eng.geometry().start_row != 0 or eng.geometry().start_col != 0  # the map did move


@pytest.mark.parametrize("batch_max", [17, 32])
@pytest.mark.parametrize("channels", ["none", "both"])
def test_quantile_ragged_batches(gpu, R, channels, batch_max):
    """The quantile estimator: eight threads per cell beyond 16 scans, the walker's chain for every row."""
    def fill(c):
        crops(c)
        c.estimation_type = 1

    scans, poses = stream(8, channels == "both", channels == "both")
    check_call(gpu, R, fill, scans, poses, batch_max)


def test_a_cropped_scan_does_not_move_the_map(gpu, R):
    """The last scan of the call has no surviving point: the map stays where the scan before it left it."""
    scans, poses = stream(9, True, False)
    scans, poses = scans[:34], poses[:34]   # scan 33 is cropped
    eng = check_call(gpu, R, crops, scans, poses, 16)
    assert eng.last_stats()[0] == 2  # FDM_SKIP_ALL_FILTERED
    short = check_call(gpu, R, crops, scans[:33], poses[:33], 16)
    assert same_geometry(eng.geometry(), short.geometry())


def test_variance_channel(gpu, R):
    """A sigma_z2 channel (pvar of the scan's record, read at the winning point).  The oracle has no such channel: batch
    launches against one launch per scan."""
    scans, poses = stream(10, True, False)
    rng = np.random.default_rng(10)
    for s in scans:
        s["sigma_z2"] = rng.uniform(1e-4, 5e-3, s["x"].size).astype(F32)
    cfg = gpu.capi.default_config()
    crops(cfg)
    a = gpu.Engine(4.0, 4.0, 0.1, cfg)
    b = gpu.Engine(4.0, 4.0, 0.1, cfg)
    b.set_option("batch", 0)
    db = DeviceBatch(gpu, scans, T(z=0.4), poses)
    assert a.integrate_device_batch(db.arr) == 0
    assert b.integrate_device_batch(db.arr) == 0
    if "tiled_min" not in gpu.Engine.default_options:
        assert sum(a.batch_launches()) >= 2
    assert a.last_stats() == b.last_stats()
    for name in b.layers():
        assert_arrays_close(a.layer(name), b.layer(name), name, 0.0, 0.0)
    assert same_geometry(a.geometry(), b.geometry())
    assert np.isfinite(a.layer("variance")).sum() > 100


def test_raycasting_ragged_batches(gpu, R):
    """raycast_enabled: the instantiations whose update resolves ray events and whose bin half captures the cloud."""
    def fill(c):
        crops(c)
        c.raycast_enabled = 1

    scans, poses = stream(11, True, False)
    eng = check_call(gpu, R, fill, scans, poses, 16, Tbs=T(z=0.6))
    assert "raycasting" in eng.layers()
