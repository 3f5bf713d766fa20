"""The owners' serial walk of the batch update (fastdem_amd/csrc/fdm_multi.hpp, mupdate_body without the ray stage) and
the tail behind it.  The walk decides its wipes by EVENT ORDINAL before the loop (a word built from the cell's scan mask
and the scans whose move vacated the cell), takes the first-sample cases of the Kalman estimator as selects, gets the
measurement variance already substituted from the exchange, and the tail wipes through a table of layer pointers in
LDS.  What can go wrong with that: a wipe at the wrong ordinal (before the first event, between two, by the scan that
then observes the cell, twice between two events, behind the last one, without any event; at bit 31), a first sample
taken for a later one or the reverse, a variance that is zero, negative, NaN or infinite, zeros of either sign as a
cell's extremes, an owner whose events straddle the two exchange rounds around a wipe, more layers than the table
holds, a layer the owner does not store but the wipe must.

Every case against the CPU oracle run scan by scan (bit-exact layers, NaN patterns, statistics), with 16 and with 32
scans per launch; the variance channel, which the oracle does not have, against the engine's own one-launch-per-scan
path and a float32 evaluation of the recursion.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from helpers import assert_arrays_close, pair
from test_batch_gpu import DeviceBatch, T, check_batch, cloud

pytestmark = pytest.mark.gpu
F32 = np.float32
RES = 0.5
JUMP = 100.0  # a move of 200 cells: more than any map here has


def _fill(estimation_type=0, mode=0):
    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 3.0, 0.0, 30.0
        c.estimation_type = estimation_type
        c.mode = mode  # 0: LOCAL (the map follows the robot), 1: GLOBAL
    return fill


def grid_scan(rng, cells, cols=None, per_cell=3, z=None, intensity=True):
    """Points of one scan in the robot's frame: `per_cell` in every cell of the rows x `cols` columns of a map of `cells`
    x `cells` cells centred on the robot (None: every column; empty: a single point that passes the crops and lies
    outside the map — the scan moves a LOCAL map and observes nothing)."""
    cols = range(cells) if cols is None else cols
    c = (np.arange(cells) - 0.5 * (cells - 1)) * RES
    x, y = np.meshgrid(c, c[list(cols)], indexing="ij")
    x, y = np.repeat(x.ravel(), per_cell), np.repeat(y.ravel(), per_cell)
    if x.size == 0:
        x, y = np.array([10.0]), np.array([0.0])
    n = x.size
    s = {"x": (x + rng.uniform(-0.2, 0.2, n)).astype(F32), "y": (y + rng.uniform(-0.2, 0.2, n)).astype(F32),
         "z": rng.choice(np.array([-0.3, -0.1, 0.0, 0.2, 0.45], dtype=F32), n) if z is None else z(n),
         "intensity": rng.uniform(0, 1, n).astype(F32) if intensity else None, "rgb": None}
    return s


def poses_of(moves):
    """One pose per character: '.' stay, 's' one cell along x, 'J' a jump of more cells than the map has."""
    out, x = [], 0.0
    for m in moves:
        x += {".": 0.0, "s": RES, "J": JUMP}[m]
        out.append(T(x, 0.0, 0.0))
    return out


def run_pattern(gpu, R, cells, batch_max, estimation_type, moves, obs, seed=1, prepare=None):
    """A lone first scan that observes every cell (it creates the layers), then ONE launch of `batch_max` scans: scan k
    moves as moves[k] says and observes the columns obs[k] selects — 'A' all, 'N' none, 'L' / 'R' the lower / upper half
    of the columns (so owners of one block see different event and wipe patterns).  A 16-character pattern is repeated
    for 32 scans: its last scan is then bit 31 of the masks."""
    eng, ref = pair(gpu, R, cells * RES, cells * RES, RES, _fill(estimation_type))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(seed)
    moves, obs = moves * (batch_max // len(moves)), obs * (batch_max // len(obs))
    assert len(moves) == len(obs) == batch_max
    half = cells // 2
    sel = {"A": None, "N": [], "L": list(range(half)), "R": list(range(half, cells))}
    first = grid_scan(rng, cells)
    check_batch(gpu, R, eng, ref, [first], T(z=0.5), [T()], expect_batches=False)
    if prepare:
        prepare(eng, ref)
    scans = [grid_scan(rng, cells, sel[o]) for o in obs]
    poses = poses_of(moves)
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), poses)
    return eng, ref


# where a cell is vacated relative to its events of the launch.  In the halves 'L' / 'R' leave out, the same move falls
# between other events (or behind the last one, or in front of the first) than in the half they observe.
WIPES = {
    "before_the_first_event":        ("J...............", "NAAAAAAAAAAAAAAA"),
    "before_the_first_event_late":   ("......J.........", "NNNNNNNLAAAAAAAR"),
    "between_events_0_and_1":        (".J..............", "ANAAAAAAAAAAAAAA"),
    "between_two_middle_events":     (".......J........", "AAALAAANARAAAAAA"),
    "between_the_last_two_events":   ("..............J.", "AAAAAAAAAAAAAANA"),
    "by_the_scan_that_observes_it":  (".....J.........J", "AAAAALAAAAAAAAAA"),
    "twice_between_two_events":      ("....JJ..........", "AAAANNAAAAAAAAAR"),
    "three_times_and_same_scan":     ("...JJJ..........", "ALANNARAAAAAAAAA"),
    "behind_the_last_event":         ("...........J....", "AAAAAAAAAAANNNNN"),
    "behind_the_last_event_at_end":  ("...............J", "AAAAAAAAAAAAAAAN"),
    "behind_it_for_half_the_cells":  ("...........J....", "AAAAAAAAAAALLLLL"),
    "without_any_event":             (".......J........", "NNNNNNNNNNNNNNNN"),
    "without_any_event_in_one_half": (".......J.....J..", "LLLLLLLLLLLLLLLL"),
    "every_scan_wipes_and_observes": ("JJJJJJJJJJJJJJJJ", "AAAAAAAAAAAAAAAA"),
    "every_scan_wipes_half_observe":  ("JJJJJJJJJJJJJJJJ", "LRLRLRLRAANNLLRR"),
}


@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [16, 32])
@pytest.mark.parametrize("case", sorted(WIPES))
def test_wipe_ordinals(gpu, R, case, batch_max, estimation_type):
    moves, obs = WIPES[case]
    run_pattern(gpu, R, 8, batch_max, estimation_type, moves, obs)


SHIFTS = {
    "one_cell_every_scan":      "s" * 16,
    "every_other_scan":         ".s" * 8,
    "none_then_every_scan":     "." * 8 + "s" * 8,
    "one_jump_beyond_the_map":  "." * 6 + "J" + "." * 9,
}


@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [16, 32])
@pytest.mark.parametrize("cells", [8, 12])
@pytest.mark.parametrize("case", sorted(SHIFTS))
def test_shift_shapes(gpu, R, case, cells, batch_max, estimation_type):
    """One-cell shifts vacate one row of the map per move — a different row every time, so the owners of one block hold
    different wipe words; random clouds leave every cell its own set of scans.  12 x 12 cells: three update blocks of 64
    cells (five of 32), the last one partial."""
    eng, ref = pair(gpu, R, cells * RES, cells * RES, RES, _fill(estimation_type))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(cells + batch_max)
    moves = SHIFTS[case] * (batch_max // 16)
    scans = [cloud(rng, 40 * cells + 13 * k, 0.55 * cells * RES, intensity=True) for k in range(1 + batch_max)]
    poses = [T()] + poses_of(moves)
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), poses)


# ---------------------------------------------------------------------------------------------
# first-sample selects (Kalman)
@pytest.mark.parametrize("batch_max", [16, 32])
@pytest.mark.parametrize("obs", ["AAAAAAAAAAAAAAAA", "RNNNNNNNNNNNNNNL", "NNNNNNNNNNNNNNNA", "LRLRNNAANNNNLLRR"])
def test_first_observation_of_a_cell_inside_the_launch(gpu, R, obs, batch_max):
    """The lone first scan observes the lower half of the columns only: the cells of the upper half have never been
    observed when the launch starts — their first sample falls in the launch's scan 0, in its last scan, or somewhere
    between, beside cells whose first sample is behind them."""
    eng, ref = pair(gpu, R, 8 * RES, 8 * RES, RES, _fill(0, mode=1))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(3)
    check_batch(gpu, R, eng, ref, [grid_scan(rng, 8, list(range(4)))], T(z=0.5), [T()], expect_batches=False)
    sel = {"A": None, "N": [], "L": list(range(4)), "R": list(range(4, 8))}
    scans = [grid_scan(rng, 8, sel[o]) for o in obs * (batch_max // 16)]
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), [T()] * batch_max)


@pytest.mark.parametrize("batch_max", [16, 32])
def test_first_observation_directly_behind_a_wipe(gpu, R, batch_max):
    """A jump vacates every cell; the next observation of a cell is a first sample again — at once for one half of the
    cells, scans later for the other, and a second time at the launch's last scan."""
    run_pattern(gpu, R, 8, batch_max, 0, "...J...........J", "AAALNNRAAAAAAAAA")


STATES = {
    # layer -> value written into the cells of row 2 + 2 i .. (the other fields keep what the first scan left)
    "elevation_nan_rest_finite": {"elevation": np.nan},
    "kalman_p_nan":              {"_kalman_p": np.nan},
    "kalman_p_inf":              {"_kalman_p": np.inf},
    "kalman_p_zero":             {"_kalman_p": 0.0},
    "n_points_zero":             {"n_points": 0.0},
    "n_points_one":              {"n_points": 1.0},
    "sample_mean_nan":           {"_sample_mean": np.nan},
    "elevation_and_mean_nan":    {"elevation": np.nan, "_sample_mean": np.nan},
}


@pytest.mark.parametrize("batch_max", [16, 32])
@pytest.mark.parametrize("case", sorted(STATES))
def test_stored_state_in_front_of_the_launch(gpu, R, case, batch_max):
    """A state written through set_layer (engine and oracle alike) in every other row of the map: isnan(elevation) and
    isnan(sample_mean) are decided independently and per event, whatever the other fields hold.  One jump in the middle
    of the launch puts a true first sample behind the prepared one."""
    def prepare(eng, ref):
        for o in (eng, ref):
            for name, v in STATES[case].items():
                a = o.layer(name)
                a[::2, :] = F32(v)
                o.set_layer(name, a)

    run_pattern(gpu, R, 8, batch_max, 0, ".........J......", "AALRAAAAAAAAAAAA", prepare=prepare)


# ---------------------------------------------------------------------------------------------
def _kalman_f32(events, min_var, max_var, q):
    """Kalman::update in float32, one operation at a time (numpy rounds each to nearest, as the device does)."""
    x = P = F32(np.nan)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        for z, var in events:
            r = var if var > 0 else max_var
            if np.isnan(x):
                x, P = z, r
            else:
                P = F32(P + q)
                k = F32(P / F32(P + r))
                x = F32(x + F32(k * F32(z - x)))
                P = F32(F32(one - k) * P)
                P = min_var if P < min_var else (max_var if max_var < P else P)
    return x, P


@pytest.mark.parametrize("batch_max", [16, 32])
def test_measurement_variance_channel_extremes(gpu, R, batch_max):
    """A sigma_z2 channel that holds 0, -1, NaN, +inf, 1e-30 and 1e30 at the winning points: the substitution R = var > 0 ?
    var : max_variance (now done in the exchange) and the clamp of P at both ends, over every event of a cell.  The
    oracle has no such channel: the batch launches against one launch per scan, bit for bit, and elevation / _kalman_p
    of every cell against the recursion evaluated in float32."""
    cfg = gpu.capi.default_config()
    _fill(0, mode=1)(cfg)
    a = gpu.Engine(8 * RES, 8 * RES, RES, cfg)
    b = gpu.Engine(8 * RES, 8 * RES, RES, cfg)
    a.set_option("batch_max", batch_max)
    b.set_option("batch", 0)
    rng = np.random.default_rng(17)
    var = np.array([2e-3, 0.0, -1.0, np.nan, np.inf, 1e-30, 1e30, 5e-4], dtype=F32)
    n_scans = 1 + batch_max
    scans, zs = [], []
    for k in range(n_scans):
        s = grid_scan(rng, 8, per_cell=1, z=lambda n: rng.uniform(-1.0, 1.0, n).astype(F32))
        s["sigma_z2"] = np.full(s["x"].size, var[k % var.size], dtype=F32)
        scans.append(s)
        zs.append(s["z"])
    db = DeviceBatch(gpu, scans, T(), [T()] * n_scans)
    before = sum(a.batch_launches())
    assert a.integrate_device_batch(db.arr) == 0
    if "tiled_min" not in gpu.Engine.default_options:  # (that fixture variant sends every scan through the record pools)
        assert sum(a.batch_launches()) > before, "the call took no batch launch"
    assert b.integrate_device_batch(db.arr) == 0
    assert a.last_stats() == b.last_stats()
    for n in b.layers():
        assert_arrays_close(a.layer(n), b.layer(n), n, 0.0, 0.0)
    # one point per cell and identity transforms: the cell's observation of scan k is that point's z.  Point j of a scan
    # lies in cell (row j // 8, column j % 8) of grid_scan's mesh: compare as sorted multisets of (elevation, P) pairs,
    # which does not depend on how the map orders its cells
    want = sorted(tuple(float(v) for v in _kalman_f32([(zs[k][j], var[k % var.size]) for k in range(n_scans)],
                                                      F32(cfg.kalman_min_variance), F32(cfg.kalman_max_variance),
                                                      F32(cfg.kalman_process_noise))) for j in range(64))
    got = sorted(zip(a.layer("elevation").ravel().astype(float).tolist(), a.layer("_kalman_p").ravel().astype(float).tolist()))
    assert got == want


@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [16, 32])
def test_zeros_of_either_sign_and_the_crop_bounds(gpu, R, batch_max, estimation_type):
    """z of +0.0 and -0.0 alternating as a cell's minimum and maximum across scans, z exactly at z_min and z_max
    (identity transforms: cropZ sees the same number), intensity +0, -0 and NaN — as a cell's first point too."""
    eng, ref = pair(gpu, R, 8 * RES, 8 * RES, RES, _fill(estimation_type, mode=1))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(23)
    sets = [np.array([0.0, -0.0], dtype=F32), np.array([-0.0, 0.0, 0.25], dtype=F32), np.array([-0.0], dtype=F32),
            np.array([0.0], dtype=F32), np.array([-2.0, 3.0, 0.0, -0.0], dtype=F32), np.array([-0.25, -0.0, 0.0], dtype=F32)]
    ints = np.array([0.0, -0.0, np.nan, 0.5, 0.75], dtype=F32)
    scans = []
    for k in range(1 + batch_max):
        zset = sets[k % len(sets)]
        s = grid_scan(rng, 8, per_cell=4, z=lambda n: rng.choice(zset, n))
        s["intensity"] = rng.choice(ints, s["x"].size)
        s["intensity"][::4] = ints[k % 3]  # the first point of every cell: +0, -0, NaN in turn
        scans.append(s)
    check_batch(gpu, R, eng, ref, scans, T(), [T()] * (1 + batch_max))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [16, 32])
@pytest.mark.parametrize("move", ["J", "s"])
@pytest.mark.parametrize("short_corner", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_state_carried_over_the_round_boundary_around_a_wipe(gpu, R, short_corner, move, batch_max, estimation_type):
    """Every cell of an 8 x 8 LOCAL map hit by every scan: 1 024 events per block, two exchange rounds.  One corner cell
    — whichever is the first in memory order — misses the second half of the scans, so event 512 falls inside a cell,
    at the ordinal of its first event behind the move in the middle of the launch: the owner carries state, wipe word
    and event count from round one into round two, and a jump vacates that cell exactly between the two rounds (a
    one-cell shift vacates one row instead)."""
    eng, ref = pair(gpu, R, 8 * RES, 8 * RES, RES, _fill(estimation_type))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(31)
    mid = batch_max // 2
    moves = "." * mid + move + "." * (batch_max - mid - 1)
    c = (np.arange(8) - 3.5) * RES
    scans = []
    for k in range(1 + batch_max):
        s = grid_scan(rng, 8)
        if k > mid:  # (scan k of the call is scan k - 1 of the launch)
            gx, gy = np.repeat(np.repeat(c, 8), 3), np.repeat(np.tile(c, 8), 3)
            keep = ~((np.sign(gx) == short_corner[0]) & (np.abs(gx) > 1.5) & (np.sign(gy) == short_corner[1]) & (np.abs(gy) > 1.5))
            s = {n: (v[keep] if v is not None else None) for n, v in s.items()}
        scans.append(s)
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), [T()] + poses_of(moves))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [16, 32])
@pytest.mark.parametrize("extra", [3, 60])
def test_wipe_of_more_layers_than_the_table_holds(gpu, R, extra, batch_max, estimation_type):
    """Plain layers added until the engine has about 70 (the LDS table of layer pointers holds 64: it is full and the
    scalar loop takes the rest; with 3 extra layers the table is partly filled), every one holding a number in every
    cell.  One-cell shifts (fewer than the map has rows): a vacated cell is NaN in all of them, every other cell keeps
    its number."""
    def prepare(eng, ref):
        for o in (eng, ref):
            for i in range(extra):
                o.add("extra_%02d" % i, 1.0 + i)
        assert len(eng.layers()) == len(ref.layers())
        assert (len(eng.layers()) > 64) == (extra == 60)

    eng, ref = run_pattern(gpu, R, 8, batch_max, estimation_type, "..s.......s.....", "AALRNAAAAAAANNLA", prepare=prepare)
    last = eng.layer("extra_%02d" % (extra - 1))
    assert np.isnan(last).any() and (last == F32(extra)).any()


@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("batch_max", [16, 32])
def test_scans_without_intensity_on_a_map_with_the_layer(gpu, R, batch_max, estimation_type):
    """The first scan carries intensity and creates the layer; the launch's scans carry none.  Their owners do not store
    the layer — the wipe of a vacated cell must (it is one of the plain layers), and every other cell keeps its value."""
    eng, ref = pair(gpu, R, 8 * RES, 8 * RES, RES, _fill(estimation_type))
    eng.set_option("batch_max", batch_max)
    rng = np.random.default_rng(41)
    check_batch(gpu, R, eng, ref, [grid_scan(rng, 8)], T(z=0.5), [T()], expect_batches=False)
    moves = ("..s.........s..." * 2)[:batch_max]
    obs = ("AALRNAAAAAAANNLA" * 2)[:batch_max]
    sel = {"A": None, "N": [], "L": list(range(4)), "R": list(range(4, 8))}
    scans = [grid_scan(rng, 8, sel[o], intensity=False) for o in obs]
    check_batch(gpu, R, eng, ref, scans, T(z=0.5), poses_of(moves))
    a = eng.layer("intensity")
    assert np.isnan(a).any() and np.isfinite(a).any()
