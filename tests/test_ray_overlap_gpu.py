"""Option ray_overlap on streams that MIX the ways a raycasting stage runs, engine against the ORACLE, bit for bit.

A scan's stage (voxel filter, ray queue, walk, resolve) runs one of three ways here:

  * S — at most `voxel_small_max` points: the sort-free voxel filter, the whole stage on the main stream (normal path);
  * M — above that, under `ray_large_min`: the library sort, the whole stage on the main stream (normal path);
  * L — at least `ray_large_min` points: voxel filter, queue and walk leave EARLY on the ray stream of the scan's parity,
    in that parity's set of buffers ("bank"), when the option allows it — `ray_overlap` 1: every enqueue-only and
    synchronous scan; `ray_overlap` -1: synchronous calls and scans of >= 1 M points (the others take the normal path).

The normal path uses bank 0, the buffers of the early stages of even scans.  A normal-path stage held back with scan k
runs on the main stream behind scan k+1's bin half; when scan k+1 is an even L scan its early stage leaves right behind
that same bin half — the two stages must not share the buffers at the same time (fdm_engine_ray.inl, run_held_ray_stage
and start_ray_stage_early).  The streams below walk every transition between the three kinds, in both orders and at both
parities of the L scan, through every entry point, and a long enqueue-only run of normal -> early transitions with no
sync between them (M scans just under `ray_large_min`: their sort and walk take the longest of the normal path).

The thresholds are lowered by engine options (set explicitly: they hold in both fixture variants) so that the oracle
keeps up.  Ghost blocks planted with `set_layer`, the same on both sides, give the stages cells to clear.
"""
import itertools

import numpy as np
import pytest

from helpers import assert_layers_bit_identical, same_geometry
from test_batch_gpu import DeviceBatch

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZE, RES = 24.0, 0.1                     # 240 x 240 cells, LOCAL map
VOXEL_SMALL_MAX, RAY_LARGE_MIN = 4096, 20000
GROWING = [20000, 20000, 40000, 40000, 20000, 60000, 60000]   # L scans: a bank holds n + n/4 + 1024 points
BIG = 1000000                             # ray_overlap -1 sends enqueue-only scans from this size up early
SENSOR_Z = 1.1
WIDE_REPEATS = 15                         # (M L S M L) x 15: 30 normal -> early transitions, half of them at each parity


def size_of(kind, rng):
    if kind in ("S", "e"):               # e: an S-sized scan whose every point is filtered away
        return int(rng.integers(2000, VOXEL_SMALL_MAX + 1))
    if kind == "M":                      # just under the threshold: the longest normal-path stage
        return int(rng.integers(RAY_LARGE_MIN - 1200, RAY_LARGE_MIN))
    if kind in ("L", "E"):               # E: the same, L-sized
        return int(rng.integers(RAY_LARGE_MIN, 60000))
    assert kind == "B"
    return BIG


def cloud(kind, rng, n=None):
    n = size_of(kind, rng) if n is None else n
    x = rng.uniform(-11.0, 11.0, n).astype(F32)
    y = rng.uniform(-11.0, 11.0, n).astype(F32)
    z = (rng.uniform(-0.6, 0.5, n) - SENSOR_Z).astype(F32)
    if kind in ("E", "e"):
        z[:] = F32(50.0)                 # cropZ drops every point: no move, no update, the stage finds nothing
    return {"x": x, "y": y, "z": z, "intensity": rng.uniform(0, 1, n).astype(F32), "kind": kind}


def pair_kinds(first_scan_no):
    """Every ordered pair of S, M, L, each with its L scan (the second scan if neither is L) at an even and at an odd
    scan number: an S scan in front moves a pair by one."""
    seq = []
    for a, b in itertools.product("SML", repeat=2):
        at = 0 if a == "L" else 1
        for want in (0, 1):
            if (first_scan_no + len(seq) + at) % 2 != want:
                seq.append("S")
            seq += [a, b]
    return seq


def plan(overlap, lead):
    """The stream: a list of groups, each a list of steps (what, kinds).  what: "one" = one enqueue-only call per scan,
    "batch" = the scans in one enqueue-only call, "sync" = the synchronous host call, "flush" = eng.sync(),
    "read" = layer reads (compared on the spot).  After every group: every layer, geometry, statistics."""
    groups = [[("one", ["S"] * lead + ["L"])]]                     # the first L scan lands at scan number `lead`
    groups.append([("one", pair_kinds(lead + 1))])
    groups.append([("one", ["L", "L"]), ("one", ["L", "L", "M", "L"]), ("one", ["L", "E", "L", "e", "L"])])
    groups.append([("batch", ["S", "S", "S"]), ("one", ["L"]), ("batch", ["S", "S"]), ("one", ["M", "L"]),
                   ("batch", ["S", "S", "L", "S", "S"]), ("one", ["L"])])
    groups.append([("one", ["L"]), ("sync", ["M"]), ("one", ["M"]), ("sync", ["L"]), ("one", ["L"]), ("sync", ["L"]),
                   ("one", ["S"]), ("sync", ["L"]), ("one", ["M"]), ("sync", ["M"])])
    groups.append([("one", ["L", "M"]), ("flush", []), ("one", ["L"]), ("read", []), ("one", ["M", "L"])])
    groups.append([("one", ["M", "L", "S", "M", "L"] * WIDE_REPEATS)])
    if overlap < 0:   # (-1: from an enqueue-only call only scans of >= 1 M points leave early: one at an even number
        n = sum(len(kinds) for g in groups for _, kinds in g)   # right behind an M scan's stage, one behind an S scan's)
        big = ["M", "B"] if n % 2 == 1 else ["S", "M", "B"]
        groups.append([("one", big + ["S", "B"])])
    return groups


def path_of(kind, overlap, sync):
    """How a scan's stage runs (start_ray_stage_early's conditions): "early" or "normal"; "none" without points."""
    if kind in ("E", "e"):
        return "early" if kind == "E" and (overlap > 0 or sync) else "none"
    if kind in ("S", "M"):
        return "normal"
    return "early" if overlap > 0 or sync or kind == "B" else "normal"


def scans_of(groups, overlap):
    """(scan number, kind, path, entry point) for every scan of the stream."""
    out, k = [], 0
    for g in groups:
        for what, kinds in g:
            for kind in kinds:
                # (a batch call's S scans ride in one launch with a stage of their own, in buffers of their own)
                path = "batch" if what == "batch" and kind == "S" else path_of(kind, overlap, what == "sync")
                out.append((k, kind, path, what))
                k += 1
    return out


def plant_ghosts(o, seed):
    """Phantom blocks in the map for the rays to pass under and clear."""
    r = np.random.default_rng(seed)
    e = o.layer("elevation").copy()
    rows, cols = e.shape
    for _ in range(6):
        r0, c0 = int(r.integers(10, rows - 18)), int(r.integers(10, cols - 18))
        e[r0:r0 + 8, c0:c0 + 8] = F32(1.25)
    o.set_layer("elevation", e)


def cfg_fill(c):
    c.z_min, c.z_max, c.range_min, c.range_max = -2.0, 4.0, 0.2, 14.0
    c.raycast_enabled = 1
    c.rc_log_odds_ghost, c.rc_clear_threshold, c.rc_height_conflict_threshold = 0.9, -0.5, 0.02
    return c


def make_pair(gpu, R, overlap):
    eng = gpu.Engine(SIZE, SIZE, RES, cfg_fill(gpu.capi.default_config()))   # (no cell ids: the batch path stays open)
    ref = R.RefEngine(SIZE, SIZE, RES, cfg_fill(R.default_config()))
    eng.set_option("ray_overlap", overlap)
    eng.set_option("ray_large_min", RAY_LARGE_MIN)
    eng.set_option("voxel_small", 1)
    eng.set_option("voxel_small_max", VOXEL_SMALL_MAX)
    return eng, ref


def compare(eng, ref, what, stats=None):
    eng.sync()
    assert sorted(eng.layers()) == sorted(ref.layers()), (what, eng.layers(), ref.layers())
    try:
        assert_layers_bit_identical(eng, ref)
    except AssertionError as err:
        raise AssertionError(f"{what}: {err}") from None
    assert same_geometry(eng.geometry(), ref.geometry()), what
    if stats is not None:
        assert eng.last_stats() == stats, (what, eng.last_stats(), stats)


@pytest.mark.parametrize("lead", [0, 1], ids=["first_L_even", "first_L_odd"])
@pytest.mark.parametrize("overlap", [1, -1])
def test_mixed_stage_kinds_against_the_oracle(gpu, R, overlap, lead):
    eng, ref = make_pair(gpu, R, overlap)
    rng = np.random.default_rng(4242 + 10 * overlap + lead)
    Tbs = np.eye(4)
    Tbs[2, 3] = SENSOR_Z
    pose = [0.0, 0.0]
    scan_no, cleared, rays_max, keep = 0, 0, 0, []

    def next_pose():
        pose[0] += float(rng.uniform(-0.25, 0.35))   # a move of up to a few cells with every scan
        pose[1] += float(rng.uniform(-0.2, 0.2))
        T = np.eye(4)
        T[0, 3], T[1, 3] = pose
        return T

    for gi, group in enumerate(plan(overlap, lead)):
        if "elevation" in ref.layers():
            for o in (eng, ref):
                plant_ghosts(o, 77 + gi)
        stats = None
        for si, (what, kinds) in enumerate(group):
            where = f"ray_overlap {overlap}, group {gi}, step {si} ({what} {''.join(kinds)}), scan {scan_no}"
            if what == "flush":
                eng.sync()
                continue
            if what == "read":
                for name in ("elevation", "raycasting", "_visibility_logodds", "ghost_removal"):
                    try:
                        assert_layers_bit_identical(eng, ref, names=[name])
                    except AssertionError as err:
                        raise AssertionError(f"{where}: {err}") from None
                continue
            scans = [cloud(k, rng) for k in kinds]
            poses = [next_pose() for _ in kinds]
            for s, T in zip(scans, poses):
                stats = ref.integrate(s["x"], s["y"], s["z"], Tbs, T, intensity=s["intensity"])
                if s["kind"] not in ("E", "e"):
                    st = ref.last_ray_stats()
                    cleared += st["n_cleared"]
                    rays_max = max(rays_max, st["n_rays"])
            if what == "sync":
                s = scans[0]
                got = eng.integrate(s["x"], s["y"], s["z"], Tbs, poses[0], intensity=s["intensity"])
                assert got == stats, (where, got, stats)
            elif what == "batch":
                b = DeviceBatch(gpu, scans, Tbs, poses)
                keep.append(b)
                assert eng.integrate_device_batch(b.arr) == 0, where
            else:
                b = DeviceBatch(gpu, scans, Tbs, poses)
                keep.append(b)
                for k in range(len(scans)):
                    one = (gpu.capi.FdmDeviceScan * 1)(b.arr[k])
                    assert eng.integrate_device_batch(one) == 0, where
            scan_no += len(kinds)
        compare(eng, ref, f"ray_overlap {overlap}, after group {gi} (scan {scan_no})", stats)
        keep.clear()   # (the stream has drained: the device arrays are dead)
    compare(eng, ref, f"ray_overlap {overlap}, at the end ({scan_no} scans)")
    # the stages did work: rays walked, ghost cells cleared
    assert rays_max > 10000, rays_max
    assert cleared > 0, "no ghost cell cleared in the whole stream"


@pytest.mark.parametrize("lead", [0, 1], ids=["first_L_even", "first_L_odd"])
@pytest.mark.parametrize("overlap", [1, -1])
def test_the_stream_reaches_every_transition(overlap, lead):
    """No engine counter tells which path a stage took (and none is added for a test), so this checks the stream's
    DEFINITION against start_ray_stage_early's conditions, which `path_of` restates: a scan's stage leaves early iff
    raycasting is on, the option wants it (1: always; -1: synchronous calls and scans of >= 1 M points), the scan was held
    back with its update (a plain scan: every scan of this stream but the batch calls' small ones), it has at least
    `ray_large_min` points and more than `voxel_small_max` (the sort-free filter keeps state of its own), and the map
    has an elevation layer (the scan's own update makes it).  All-filtered L-sized scans leave too: the stage finds
    nothing.  Everything else runs on the main stream, in bank 0.  Asserted: every ordered pair of S, M, L at both
    parities of the L scan, normal -> early into bank 0, batch calls on either side of an early stage, an all-filtered
    scan between two L scans, a flush and a layer read mid-stream, and under option 1 at least 24 normal -> early
    transitions in one enqueue-only run, at least 12 of them into bank 0."""
    groups = plan(overlap, lead)
    scans = scans_of(groups, overlap)
    assert next(k for k, kind, _, _ in scans if kind == "L") == lead
    seen = {(a, b, k1 % 2, pa, pb) for (_, a, pa, _), (k1, b, pb, _) in zip(scans, scans[1:])}
    for a, b in itertools.product("SML", repeat=2):
        for par in (0, 1):   # (parity of the second scan)
            assert any(x[:3] == (a, b, par) for x in seen), (a, b, par)
    if overlap > 0:
        assert any(x[3:] == ("normal", "early") and x[2] == 0 for x in seen)
        assert any(x[3:] == ("batch", "early") for x in seen) and any(x[3:] == ("early", "batch") for x in seen)
        k0 = sum(len(kinds) for g in groups[:-1] for _, kinds in g)
        assert groups[-1] == [("one", ["M", "L", "S", "M", "L"] * WIDE_REPEATS)]
        run = scans[k0:]
        into = [b[0] % 2 for a, b in zip(run, run[1:]) if a[2] == "normal" and b[2] == "early"]
        assert len(into) >= 24 and into.count(0) >= 12, into
    else:
        # -1: the normal path everywhere but the synchronous L calls (behind a flush of what came before) and the
        # 1 M-point scans — one of them an even scan right behind an M scan's held-back stage
        assert ("M", "B", 0, "normal", "early") in seen and ("S", "B", 0, "normal", "early") in seen
        assert any(p == "early" and w == "sync" for _, _, p, w in scans)
    assert any(w == "flush" for g in groups for w, _ in g) and any(w == "read" for g in groups for w, _ in g)
    assert any(kind == "E" and scans[k - 1][1] == "L" and scans[k + 1][1] == "L" for k, kind, _, _ in scans)
    assert ("L", "L", 1, "early", "early") in seen or ("L", "L", 0, "early", "early") in seen or overlap < 0


@pytest.mark.parametrize("any_order", [0, 1], ids=["stable_order", "std_sort_order"])
def test_banks_grow_under_a_held_stage(gpu, R, any_order):
    """Both banks are allocated (scans 0, 1) and then grown twice (scans 2, 3 and 5, 6) by start_ray_stage_early while
    the previous scan's stage is held back with its update: the allocation drains the streams, which flushes the held
    stage AND the scan being enqueued (run_held_ray_stage, bank 0) before anything of its early part is launched.  With
    `voxel_any_order` 1 the bank's introsort buffer grows with it; the oracle then sorts with std::sort
    (tests/test_voxel_order_gpu.py).  One enqueue-only call per scan, nothing waits before the layer read in the
    middle and the end."""
    caps = [0, 0]
    grown = [0, 0]
    for k, n in enumerate(GROWING):      # the stream's definition: every bank allocated once, grown twice
        if n > caps[k % 2]:
            grown[k % 2] += 1
            caps[k % 2] = n + n // 4 + 1024
    assert grown == [3, 3] and min(GROWING) >= RAY_LARGE_MIN > VOXEL_SMALL_MAX
    eng, ref = make_pair(gpu, R, 1)
    eng.set_option("voxel_any_order", any_order)
    ref.set_voxel_stable(not any_order)
    rng = np.random.default_rng(99 + any_order)
    Tbs = np.eye(4)
    Tbs[2, 3] = SENSOR_Z
    keep, stats, cleared = [], None, 0
    for k, n in enumerate(GROWING):
        s = cloud("L", rng, n)
        T = np.eye(4)
        T[0, 3], T[1, 3] = 0.3 * k, -0.15 * k
        stats = ref.integrate(s["x"], s["y"], s["z"], Tbs, T, intensity=s["intensity"])
        cleared += ref.last_ray_stats()["n_cleared"]
        b = DeviceBatch(gpu, [s], Tbs, [T])
        keep.append(b)
        assert eng.integrate_device_batch(b.arr) == 0, k
        if k == 3:                       # both banks have grown once: a layer read, no sync ahead of it
            where = f"voxel_any_order {any_order}, layer read behind scan {k}"
            try:
                assert_layers_bit_identical(eng, ref)
            except AssertionError as err:
                raise AssertionError(f"{where}: {err}") from None
            assert same_geometry(eng.geometry(), ref.geometry()), where
            assert eng.last_stats() == stats, (where, eng.last_stats(), stats)
            for o in (eng, ref):
                plant_ghosts(o, 5)
    compare(eng, ref, f"voxel_any_order {any_order}, at the end", stats)
    assert cleared > 0, "no ghost cell cleared behind the planted blocks"
