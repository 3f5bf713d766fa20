"""The flush of the batch pipeline's bin half (fastdem_amd/csrc/fdm_multi.hpp, mbin_body) and the decode at the other end
(mupd_exchange): a record's aux words — the cell's maximum z, maximum intensity, first point, colour slot — leave in ONE
atomic maximum from four adjacent lanes, the first point inverted so that every word is a maximum and the clean scratch is
all zeros; the key half of a record goes through one wavefront per pass of 64 records.

What can go wrong: a word in the wrong lane, the first point decoded without its inverse (the NaN flag is its lowest bit),
a word of value 0 that needed no atomic but was expected (point 0 with a finite intensity, a cell of NaN intensities, a
maximum z at the lowest float), a block that is not the cell's only one (minimum, maxima, first and last point in different
blocks), the passes' boundaries (63, 64, 65, 128, 512 records of a block), the scratch re-armed with another clean value than
the one the flush and the next batch but one expect, a channel the instantiation does not have.

Every case against the CPU oracle run scan by scan, bit for bit (layers, geometry, statistics of the last scan; the
oracle's answers of a case are computed once and shared by its variants), with the Kalman estimator (16 scans per launch)
and the quantile estimator (32), and the batch scratch must read clean after every call.  Identity transforms and a map
that never moves (48 x 48 cells of 0.25 m: 4.5 rounds of the 512-slot table), so a point's cell is known here; block b of
a scan holds points [512 b, 512 b + 512).

Run on the GPU box:  python -m pytest tests -m gpu
"""
import zlib

import numpy as np
import pytest

from helpers import assert_layers_bit_identical, pair, same_geometry
from test_batch_gpu import T, check_batch
from test_batch_bin_claim_gpu import RES, SIDE, _Oracle, at_cells, glue, outside

pytestmark = pytest.mark.gpu
F32 = np.float32
NAN = float("nan")
ESTS = [0, 1]
NCELL = SIDE * SIDE


def per_launch(est):
    return 32 if est == 1 else 16


def _fill(est, ray):
    def fill(c):
        c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 3.0, 0.0, 60.0
        c.estimation_type = est
        c.mode = 0
        c.raycast_enabled = int(ray)
    return fill


def rng_of(key, est):
    return np.random.default_rng(zlib.crc32(key.encode()) + est)


def run(gpu, R, key, est, calls, ray=False, twice=False, poses=None, Tbs=None):
    """`calls`: lists of scans, one fdm_engine_integrate_device_batch each (the first scan of a fresh engine goes alone),
    on one map; the scratch must be clean behind every call.  twice: the same calls on a second fresh engine, bit for bit."""
    Tbs = T() if Tbs is None else Tbs
    eng, ref = pair(gpu, R, SIDE * RES, SIDE * RES, RES, _fill(est, ray))
    other = pair(gpu, R, SIDE * RES, SIDE * RES, RES, _fill(est, ray))[0] if twice else None
    orc = _Oracle(("flush_" + key, est), ref)
    at = 0
    for scans in calls:
        ps = [T() for _ in scans] if poses is None else poses[at:at + len(scans)]
        at += len(scans)
        orc.call(len(scans))
        check_batch(gpu, R, eng, orc, scans, Tbs, ps)
        assert eng.debug_batch_dirty() == (0, 0, 0)   # (it waits for everything enqueued: a sync between two calls)
        if other is not None:
            orc.call(len(scans), again=True)
            check_batch(gpu, R, other, orc, scans, Tbs, ps)
            assert_layers_bit_identical(other, eng)
            assert same_geometry(other.geometry(), eng.geometry())
    orc.done()
    return eng


def away_from(rng, n, avoid):
    """n points anywhere on the map but in the cells `avoid`."""
    allowed = np.setdiff1d(np.arange(NCELL), np.asarray(avoid))
    return at_cells(rng, rng.choice(allowed, n))


def put(s, i, cell, z, inten=None, rgb=None):
    """Point i of the scan into the centre of `cell` (row + SIDE * column, row 0 at the highest x)."""
    r, c = cell % SIDE, cell // SIDE
    s["x"][i] = F32((0.5 * SIDE - r - 0.5) * RES)
    s["y"][i] = F32((0.5 * SIDE - c - 0.5) * RES)
    s["z"][i] = F32(z)
    if inten is not None:
        s["intensity"][i] = F32(inten)
    if rgb is not None:
        s["rgb"][i] = np.uint32(rgb)


def channels(scans, ch):
    for s in scans:
        if ch in ("none", "colour"):
            s["intensity"] = None
        if ch in ("none", "intensity"):
            s["rgb"] = None
    return scans


# ---------------------------------------------------------------------------------------------
def _three_blocks(variant, est):
    """Cell C of scan k: its first point in block 0, and minimum z, maximum z and maximum intensity spread over blocks 1
    and 2 in an order that turns with k."""
    rng = rng_of("three_" + variant, est)
    scans = [away_from(rng, 700, [])]
    for k in range(per_launch(est)):
        C = 1000 + 7 * k
        s = away_from(rng, 1300, [C])
        b_min, b_max, b_int = [(1, 2, 1), (2, 1, 2), (1, 2, 2), (2, 1, 1)][k % 4]
        put(s, 7, C, 0.1, NAN if variant == "first_nan" else 0.3, 0x010203)          # the cell's first point
        put(s, 300, C, 0.15, 0.4, 0x111111)
        if variant == "later_block_nan":
            put(s, 512 + 10, C, 0.0, NAN, 0x222222)                                     # block 1's first point of C
        put(s, 512 * b_min + 40, C, -0.4, 0.2, 0x333333)
        put(s, 512 * b_max + 100, C, 0.6, 0.1, 0x444444)
        put(s, 512 * b_int + 200, C, 0.05, 0.95, 0x555555)
        scans.append(s)
    return [scans]


@pytest.mark.parametrize("est", ESTS)
@pytest.mark.parametrize("variant", ["first_nan", "first_finite", "later_block_nan"])
def test_one_cell_fed_by_three_blocks(gpu, R, variant, est):
    run(gpu, R, "three_" + variant, est, _three_blocks(variant, est))


# ---------------------------------------------------------------------------------------------
E = [40 + 49 * j for j in range(8)]  # the edge cells


def _edges(est):
    rng = rng_of("edges", est)
    scans = [away_from(rng, 700, E)]
    for k in range(per_launch(est)):
        s = away_from(rng, 600, E)
        put(s, 0, E[0], 0.2, NAN if k % 2 == 0 else 0.5)      # point 0: fst = 1 / fst = 0 (no atomic at all)
        for i in (20, 530, 540):
            put(s, i, E[1], 0.1 + 0.001 * i, NAN)             # every intensity NaN: imx = 0
        put(s, 30, E[2], -0.2, -0.5); put(s, 31, E[2], 0.0, 0.0)        # maxima +0.0
        put(s, 32, E[3], -0.2, -0.5); put(s, 33, E[3], -0.0, -0.0)      # maxima -0.0
        put(s, 40, E[4], 0.0, 0.0); put(s, 550, E[4], -0.0, -0.0)       # +0 first, -0 in the next block
        put(s, 41, E[5], -0.0, -0.0); put(s, 551, E[5], 0.0, 0.0)       # -0 first
        put(s, 42, E[6], -0.0, -0.0)                                      # alone
        put(s, 599, E[7], 0.0, NAN)                                       # the scan's last point, in the ragged block
        scans.append(s)
    return [scans]


@pytest.mark.parametrize("est", ESTS)
def test_words_at_their_edges(gpu, R, est):
    run(gpu, R, "edges", est, _edges(est))


@pytest.mark.parametrize("est", ESTS)
def test_a_maximum_at_the_lowest_float(gpu, R, est):
    """Every second scan stands at z = -FLT_MAX: its points reach the map at the lowest float, which is no maximum
    (strict '>' from lowest()): the word is 0 and leaves no atomic, the key still does."""
    rng = rng_of("lowest", est)
    n = 1 + per_launch(est)
    scans = [away_from(rng, 300 if k else 700, []) for k in range(n)]
    poses = [T(z=-3.4028234663852886e38) if k % 2 == 0 and k else T() for k in range(n)]
    run(gpu, R, "lowest", est, [scans], poses=poses)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTS)
@pytest.mark.parametrize("records", [0, 1, 63, 64, 65, 128, 512])
def test_records_per_block(gpu, R, records, est):
    """Block 0 of every scan holds `records` cells (the passes of the four-lane part take 64 records each), block 1 is
    ragged and meets some of them again."""
    rng = rng_of("records_%d" % records, est)
    scans = [away_from(rng, 700, [])]
    for k in range(per_launch(est)):
        if records == 0:
            b0 = outside(rng, 512)
        else:
            own = rng.permutation(NCELL)[:records]
            b0 = at_cells(rng, np.concatenate([own, own[rng.integers(0, records, 512 - records)]]))
        scans.append(glue(b0, away_from(rng, 90 + k, [])))
    run(gpu, R, "records_%d" % records, est, [scans])


# ---------------------------------------------------------------------------------------------
def _channel_scans(est, key):
    rng = rng_of(key, est)
    scans = [away_from(rng, 700, [])]
    for k in range(per_launch(est)):
        C = 300 + 11 * k
        s = away_from(rng, 1300, [C])
        put(s, 50, C, -0.5, 0.3, 0xAA0000)           # the winner: block 0
        put(s, 700, C, 0.3, 0.8, 0x00BB00)
        put(s, 1024 + k, C, 0.1, 0.2, 0x0000CC + k)  # the last point, whose colour the cell takes: block 2
        scans.append(s)
    return scans


@pytest.mark.parametrize("est", ESTS)
@pytest.mark.parametrize("ch", ["none", "intensity", "colour", "both"])
def test_channel_sets(gpu, R, ch, est):
    run(gpu, R, "channels_" + ch, est, [channels(_channel_scans(est, "channels"), ch)])


# ---------------------------------------------------------------------------------------------
P = [5 + 113 * j for j in range(20)]  # the cells every scan of the reuse cases feeds


def _reuse_scans(est, n_batches):
    """Batch b feeds the cells P with extremes that SHRINK with b, a first point that comes later and a last point in an
    earlier block: a word left in the scratch by batch b would win in batch b + 2 (the same set of the scratch)."""
    rng = rng_of("reuse", est)
    scans = [away_from(rng, 700, [])]
    for b in range(n_batches):
        for k in range(per_launch(est)):
            s = away_from(rng, 1300, P)
            for j, C in enumerate(P):
                a = 0.1 * (6 - b)
                put(s, 3 + 30 * b + j, C, -a, NAN if (j + b) % 3 == 0 else 0.9 - 0.2 * b, 0x100 * b + j)
                put(s, 400 + j, C, a, 0.05, 0x200 * b + j)
                if b < 2:
                    put(s, 600 + j, C, 0.0, 0.1, 0x300 * b + j)
                    put(s, 1100 + j, C, -0.0, 0.02, 0x400 * b + j)
            scans.append(s)
    return scans


@pytest.mark.parametrize("est", ESTS)
@pytest.mark.parametrize("shape", ["three_launches", "four_launches", "two_calls"])
def test_scratch_reuse(gpu, R, shape, est):
    scans = _reuse_scans(est, 4)
    nb = per_launch(est)
    if shape == "three_launches":
        calls = [scans[:1 + 3 * nb]]
    elif shape == "four_launches":
        calls = [scans]
    else:
        calls = [scans[:1 + 2 * nb], scans[1 + 2 * nb:]]
    run(gpu, R, "reuse_" + shape, est, calls)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTS)
@pytest.mark.parametrize("n_scans", [2, 16, 17, 32])
def test_scans_per_call(gpu, R, n_scans, est):
    rng = rng_of("scans_%d" % n_scans, est)
    scans = [away_from(rng, int(rng.integers(300, 1300)), []) for _ in range(1 + n_scans)]
    run(gpu, R, "scans_%d" % n_scans, est, [scans])


def test_with_raycasting(gpu, R):
    """The ray instantiations share the flush."""
    rng = rng_of("ray", 0)
    scans = channels([away_from(rng, int(rng.integers(300, 1300)), []) for _ in range(1 + 17)], "intensity")
    run(gpu, R, "ray", 0, [scans], ray=True, Tbs=T(z=0.5))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTS)
def test_the_same_calls_on_two_engines_leave_the_same_bits(gpu, R, est):
    run(gpu, R, "three_later_block_nan", est, _three_blocks("later_block_nan", est), twice=True)
    run(gpu, R, "channels_both", est, [_channel_scans(est, "channels")], twice=True)
