"""The bin half of the batch pipeline (fastdem_amd/csrc/fdm_multi.hpp, mbin_body): the chain of LOCAL-mode moves and the
fold of a block's points into its LDS cell table.

The chain.  Lane j of the block's first wavefront rounds scan j's pose once against the chain's start, and scan j's own
shift is that total minus the cells shifted so far — which is only valid off the rounding ties and below 1e7 m, and only
wrapped once behind the walk for moves of fewer cells than the map has; anything else takes the reference's own
arithmetic at its place in the walk.  What can go wrong: a shift taken against the wrong predecessor (holes in the pass
mask: scans whose points were all cropped do not move the map), the rounded total trusted on a tie, near one, beyond
1e7 m or on a jump of a map's length, the start index wrapped wrongly behind a long chain, the previous batch's last
scan passing or not.

The fold.  Both points of a thread probe the table in one batch; the lane that finds a slot empty has CLAIMED it and
numbers its record there (ballot + one LDS add per wavefront), and the flush walks the records in claim order — the
record's number is the cell's slot in the scan's observation arrays.  What can go wrong: a full table whose probes wrap,
512 points in one cell, cells that share a hash slot, a wavefront that claims nothing between two that do, the second
point's claims left out of the numbering, run-merged wavefronts beside plain ones, colours and observations read through
the wrong slot.  The order of a block's records depends on timing and must not show: the same call on two fresh engines
leaves the same bits.

Every case against the CPU oracle run scan by scan (bit-identical layers, geometry, statistics; the oracle's answers
of a case are computed once and shared by its variants), with `batch_walk` -1, 0 and 1, the Kalman estimator with 16
scans per launch and the quantile estimator with 32; the chain cases also against the same call with `dbg_batch` 3 (every
move by the reference's divide), bit for bit.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from helpers import assert_layers_bit_identical, pair, same_geometry
from test_batch_gpu import T, check_batch, cloud

pytestmark = pytest.mark.gpu
F32 = np.float32
RES = 0.25              # dyadic: half-cell poses are exact rounding ties
ROWS, COLS = 24, 20     # the chain cases' map (x: rows, y: columns)
SIDE = 48               # the claim cases' map: 48 x 48 cells, 4.5 hash rounds of the 512-slot table
WALKS = [-1, 0, 1]


def _fill(estimation_type):
    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 3.0, 0.0, 60.0
        c.estimation_type = estimation_type
        c.mode = 0  # LOCAL: the map follows the robot
    return fill


def _per_launch(estimation_type):
    return 32 if estimation_type == 1 else 16


# ---------------------------------------------------------------------------------------------
# the oracle's answers, once per case
_ORACLE = {}


class _Oracle:
    """Stands where check_batch expects the reference engine.  The first test of a case runs the CPU oracle and keeps what
    check_batch reads of it behind every call (statistics of the call's last scan, layers, geometry; read-only); the
    case's other variants are checked against those."""

    def __init__(self, key, ref):
        self.key, self.ref = key, ref
        self.calls = _ORACLE.get(key)
        self.live = self.calls is None
        self.rec, self.at, self.left, self.again = [], -1, 0, False

    def call(self, n_scans, again=False):
        """The case's next call — or, again: the same call once more, for a second engine."""
        self.at, self.left, self.again = self.at + (0 if again else 1), n_scans, again

    def integrate(self, *a, **kw):
        self.left -= 1
        if not self.live or self.again:
            return self._now()[0]
        out = self.ref.integrate(*a, **kw)
        if self.left == 0:
            lay = {n: self.ref.layer(n).copy() for n in self.ref.layers()}
            for v in lay.values():
                v.setflags(write=False)
            self.rec.append((out, lay, self.ref.geometry()))
        return out

    def _now(self):
        return (self.rec if self.live else self.calls)[self.at]

    def layers(self):
        return list(self._now()[1])

    def layer(self, name):
        return self._now()[1][name]

    def geometry(self):
        return self._now()[2]

    def done(self):
        if self.live:
            _ORACLE[self.key] = self.rec


def run_case(gpu, R, key, size, estimation_type, batch_walk, calls, Tbs, position=(0.0, 0.0), against_divide=False,
             twice=False):
    """`calls`: a list of (scans, poses), one fdm_engine_integrate_device_batch each, on one map.  against_divide: the same
    calls on a second engine with dbg_batch 3, bit for bit.  twice: the same calls on a second fresh engine, bit for bit."""
    eng, ref = pair(gpu, R, size[0] * RES, size[1] * RES, RES, _fill(estimation_type), position=position)
    eng.set_option("batch_walk", batch_walk)
    other = None
    if against_divide or twice:
        other, _ = pair(gpu, R, size[0] * RES, size[1] * RES, RES, _fill(estimation_type), position=position)
        other.set_option("batch_walk", batch_walk)
        if against_divide:
            other.set_option("dbg_batch", 3)
    orc = _Oracle((key, estimation_type), ref)
    for scans, poses in calls:
        orc.call(len(scans))
        check_batch(gpu, R, eng, orc, scans, Tbs, poses)
        if other is not None:
            orc.call(len(scans), again=True)
            check_batch(gpu, R, other, orc, scans, Tbs, poses)
            assert_layers_bit_identical(other, eng)
            assert same_geometry(other.geometry(), eng.geometry())
    orc.done()
    return eng


# ---------------------------------------------------------------------------------------------
# chain cases: where scan k of the launch stands, in cells from the map's first position
def _steps(fx, fy):
    return lambda k: (fx * k, fy * k)


def _jump(jx, jy, at=5):
    """0.35 / 0.27 cell per scan, and scan `at` moves by exactly (jx, jy) cells instead of its step."""
    def f(k):
        s = k if k < at else k - 1
        return (0.35 * s + (jx if k >= at else 0), -0.27 * s + (jy if k >= at else 0))
    return f


def _near_tie(off):
    """0.35 cell per scan along x, scan 7 within 1e-4 cell of the tie at 2.5 cells (its neighbours stand at 2.1 and 2.8)."""
    return lambda k: ((2.5 + off) if k == 7 else 0.35 * k, 0.2 * k)


# name -> (pose of scan k, scans of the launch whose points are all cropped (None: see the name), start position)
CHAINS = {
    "plus_x":                    (_steps(0.35, 0.0), (), (0.0, 0.0)),
    "minus_y":                   (_steps(0.0, -0.35), (), (0.0, 0.0)),
    "diagonal":                  (_steps(0.35, -0.35), (), (0.0, 0.0)),
    "diagonal_back":             (_steps(-0.35, 0.27), (), (0.0, 0.0)),
    "half_cell_ties":            (_steps(0.5, -0.5), (), (0.0, 0.0)),
    "near_tie_below":            (_near_tie(-5e-5), (), (0.0, 0.0)),
    "near_tie_above":            (_near_tie(5e-5), (), (0.0, 0.0)),
    "jump_rows_minus_1":         (_jump(ROWS - 1, -(COLS - 1)), (), (0.0, 0.0)),
    "jump_back_rows_minus_1":    (_jump(-(ROWS - 1), COLS - 1, at=9), (), (0.0, 0.0)),
    "jump_rows":                 (_jump(ROWS, 0), (), (0.0, 0.0)),
    "jump_back_cols":            (_jump(0, -COLS, at=2), (), (0.0, 0.0)),
    "jump_two_rows":             (_jump(2 * ROWS, 0), (), (0.0, 0.0)),
    "jump_back_two_rows_cols":   (_jump(-2 * ROWS, 2 * COLS, at=11), (), (0.0, 0.0)),
    "holes_0_3_4_9":             (_steps(0.35, -0.27), (0, 3, 4, 9), (0.0, 0.0)),
    "last_scan_cropped":         (_steps(0.35, -0.27), None, (0.0, 0.0)),
    "all_but_one_cropped":       (_steps(0.35, -0.27), None, (0.0, 0.0)),
    "holes_and_a_tie":           (_steps(0.5, 0.35), (1, 2, 8), (0.0, 0.0)),
    "holes_and_a_long_jump":     (_jump(2 * ROWS, -COLS, at=6), (0, 5, 7), (0.0, 0.0)),
    "start_beyond_1e7":          (_steps(0.35, -0.27), (3,), (1.25e7 + 3 * RES, -2.5e7 - RES)),
}


def _chain_calls(case, estimation_type):
    pose_of, cropped, position = CHAINS[case]
    nb = _per_launch(estimation_type)
    if case == "last_scan_cropped":
        cropped = (nb - 1,)
    elif case == "all_but_one_cropped":
        cropped = tuple(k for k in range(nb) if k != 6)
    rng = np.random.default_rng(sorted(CHAINS).index(case) + 100 * estimation_type)
    scans, poses = [], []
    for k in range(-1, nb):  # (the first scan of a fresh engine goes alone and creates the layers; then one launch)
        s = cloud(rng, int(rng.integers(40, 1100)), 0.55 * ROWS * RES, intensity=True)
        if k in cropped:
            s["z"] = (s["z"] + 40.0).astype(F32)
        cx, cy = pose_of(max(k, 0))
        scans.append(s)
        poses.append(T(position[0] + cx * RES, position[1] + cy * RES, 0.0, yaw=0.03 * (k + 1)))
    return [(scans, poses)], position


@pytest.mark.parametrize("batch_walk", WALKS)
@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("case", sorted(CHAINS))
def test_chain_of_moves(gpu, R, case, estimation_type, batch_walk):
    calls, position = _chain_calls(case, estimation_type)
    run_case(gpu, R, "chain_" + case, (ROWS, COLS), estimation_type, batch_walk, calls, T(z=0.5), position=position,
             against_divide=True)


@pytest.mark.parametrize("batch_walk", WALKS)
@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("last_passes", [True, False])
def test_three_batches_in_one_call(gpu, R, last_passes, estimation_type, batch_walk):
    """1 + three launches in one call: the chain of batch b starts from the last scan of batch b - 1, whose candidate
    applies only if that scan had a surviving point — not so for the last scans of the first two batches, in one variant."""
    nb = _per_launch(estimation_type)
    rng = np.random.default_rng(7 + estimation_type)
    scans, poses = [], []
    for k in range(1 + 3 * nb):
        s = cloud(rng, int(rng.integers(40, 400)), 0.55 * ROWS * RES, intensity=True)
        if (not last_passes and k in (nb, 2 * nb)) or k in (3, nb + 2, 2 * nb + 5):
            s["z"] = (s["z"] + 40.0).astype(F32)
        scans.append(s)
        poses.append(T(0.35 * RES * k, -0.27 * RES * k, 0.0, yaw=0.01 * k))
    run_case(gpu, R, "three_batches_%d" % last_passes, (ROWS, COLS), estimation_type, batch_walk, [(scans, poses)], T(z=0.5),
             against_divide=True)


# ---------------------------------------------------------------------------------------------
# claim cases: identity transforms and a map that never moves, so a point's cell is known here — the cell of row r and
# column c is c * SIDE + r in the bin half's numbering (its table slot: that number modulo 512), row 0 at the highest x
ZSET = np.array([-0.3, -0.1, 0.0, -0.0, 0.2, 0.45], dtype=F32)  # few heights: equal minima everywhere


def at_cells(rng, cells):
    cells = np.asarray(cells)
    r, c = cells % SIDE, cells // SIDE
    n = cells.size
    x = (0.5 * SIDE - r - 0.5) * RES + rng.uniform(-0.4, 0.4, n) * RES
    y = (0.5 * SIDE - c - 0.5) * RES + rng.uniform(-0.4, 0.4, n) * RES
    return {"x": x.astype(F32), "y": y.astype(F32), "z": rng.choice(ZSET, n),
            "intensity": rng.choice(np.array([0.0, -0.0, np.nan, 0.5, 0.75, 0.9], dtype=F32), n),
            "rgb": rng.integers(0, 1 << 24, n, dtype=np.uint32)}


def outside(rng, n):
    """Points that pass the crops and lie beyond the map's edge."""
    s = at_cells(rng, np.zeros(n, dtype=np.int64))
    s["x"] = (s["x"] + F32(20.0)).astype(F32)
    return s


def glue(*parts):
    return {n: np.concatenate([p[n] for p in parts]) for n in parts[0]}


def anywhere(rng, n):
    return at_cells(rng, rng.integers(0, SIDE * SIDE, n))


def _table_full(rng, k):
    """Block 0: 512 points in 512 distinct cells whose table slots all start in [384, 512) — every probe sequence runs
    over the table's end, and the table ends up full."""
    cells = np.array([c for c in range(SIDE * SIDE) if c % 512 >= 384][:512])
    assert cells.size == 512 and np.unique(cells).size == 512
    return glue(at_cells(rng, rng.permutation(cells)), anywhere(rng, 150 + 7 * k))


def _one_cell(rng, k):
    return at_cells(rng, np.full(512 + 40 + k, 777 + k))


def _same_hash_slot(rng, k):
    c0 = 100 + 3 * k
    return at_cells(rng, rng.choice(np.array([c0, c0 + 512, c0 + 1024]), 600 + k))


def _sizes(rng, k):
    return anywhere(rng, [513, 1, 512, 511, 1, 1025, 40, 1100][k % 8])


def _outside_scans(rng, k):
    return outside(rng, 300 + k) if k % 5 in (2, 3) else anywhere(rng, 513)


def _empty_wavefront(rng, k):
    """Thread t holds points t and t + 256 of its block: wavefront 1 (points 64-127 and 320-383) has no point inside
    the map, its neighbours have; in the second block wavefront 2 has none and wavefront 3 only its second point."""
    s = anywhere(rng, 1024)
    o = outside(rng, 1024)
    gone = np.zeros(1024, dtype=bool)
    gone[64:128] = gone[320:384] = True
    gone[512 + 128:512 + 192] = gone[512 + 384:512 + 448] = True
    gone[512 + 192:512 + 256] = True
    for n in s:
        s[n][gone] = o[n][gone]
    return s


def _image_runs(rng, k):
    """Neighbouring points in the same cell, eight at a time (the wavefronts merge their runs in registers and only the
    run tails touch the table)."""
    return at_cells(rng, np.repeat(rng.permutation(SIDE * SIDE)[:128], 8))


def _mixed_runs(rng, k):
    """Run-merged wavefronts beside plain ones in one block, and runs of three beside runs of six inside a wavefront."""
    runs8 = np.repeat(rng.integers(0, SIDE * SIDE, 24), 8)    # points 0-191: wavefronts 0-2, first point
    plain = rng.integers(0, SIDE * SIDE, 256)                   # 192-447
    runs36 = np.concatenate([np.repeat(rng.integers(0, SIDE * SIDE, 1), n) for n in (3, 6) * 40])[:320]
    return at_cells(rng, np.concatenate([runs8, plain, runs36]))


CLAIMS = {
    "table_full_probes_wrap": _table_full,
    "every_point_in_one_cell": _one_cell,
    "three_cells_one_hash_slot": _same_hash_slot,
    "sizes_513_and_1": _sizes,
    "scans_outside_the_map": _outside_scans,
    "a_wavefront_without_inside_points": _empty_wavefront,
    "image_ordered_runs": _image_runs,
    "mixed_runs": _mixed_runs,
}


def _claim_calls(case, estimation_type):
    rng = np.random.default_rng(sorted(CLAIMS).index(case) + 50 * estimation_type)
    nb = _per_launch(estimation_type)
    scans = [anywhere(rng, 700)] + [CLAIMS[case](rng, k) for k in range(nb)]
    return [(scans, [T() for _ in scans])]


@pytest.mark.parametrize("batch_walk", WALKS)
@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("case", sorted(CLAIMS))
def test_claimed_slots(gpu, R, case, estimation_type, batch_walk):
    run_case(gpu, R, "claim_" + case, (SIDE, SIDE), estimation_type, batch_walk, _claim_calls(case, estimation_type), T())


@pytest.mark.parametrize("estimation_type", [0, 1])
@pytest.mark.parametrize("case", ["table_full_probes_wrap", "mixed_runs"])
def test_the_order_of_a_blocks_records_does_not_show(gpu, R, case, estimation_type):
    """A block's records are numbered in the order its wavefronts reach the counter: the same call on two fresh engines
    must leave the same bits in every layer."""
    run_case(gpu, R, "claim_" + case, (SIDE, SIDE), estimation_type, -1, _claim_calls(case, estimation_type), T(), twice=True)
