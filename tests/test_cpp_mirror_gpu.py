"""The C++ host mirror (fastdem_amd/cpp/include: FastDEM, ElevationMap, nanogrid::GridMap, ElevationMapping, the
postprocess wrappers) held to the oracle end to end.

Seeded scripts of map / mapper / scan / layer-access steps (tests/mirror_script.py) run through the mirror's public
C++ API in fastdem_amd/cpp/tests/mirror_replay.cpp — built twice, as users ship it (-DNDEBUG: a stale host copy reads
silently) and with the Matrix guard on (FDM_MIRROR_GUARD: it throws) — and on fdm_ref_py maps.  After every dump the
layers, every held Matrix& and the geometry are compared bit for bit; so are every returned bool, lastStats() and the
scan-callback clouds.  Every script obeys the mirror's access contract: a held reference is dereferenced only after a
host access through its map that follows the last device operation (nanogrid.hpp, Matrix::guard)."""
import os
import subprocess

import numpy as np
import pytest

import mirror_script as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "fastdem_amd", "cpp", "build")
BINS = {"ndebug": os.path.join(BUILD, "fdm_mirror_replay"), "guard": os.path.join(BUILD, "fdm_mirror_replay_guard")}
YAML = os.path.join(ROOT, "fastdem_amd", "config", "default.yaml")
FILES = {"default.yaml": YAML}


# ------------------------------------------------------------------------------------------------------ scripts ----
def _touch_and_write(s, slot, handles, rng, next_xy, layer_at="variance"):
    """One host access after the device step, then writes through held handles (one at the cell the next scan sees),
    a write through at(), and a dump."""
    s.op("touch", slot, "elevation")
    for h, v in handles:
        if h.endswith("E") or h.endswith("K"):
            s.op("hwritepos", h, MS._g(next_xy[0] + rng.uniform(-0.3, 0.3)), MS._g(next_xy[1] + rng.uniform(-0.3, 0.3)),
                 MS._g(v))
        else:
            s.op("hwrite", h, int(rng.integers(0, 200)), int(rng.integers(0, 200)), MS._g(v))
    s.op("at", slot, layer_at, int(rng.integers(0, 200)), int(rng.integers(0, 200)), MS._g(rng.uniform(0.001, 0.01)))
    s.op("dump", slot)


def script_handles(seed=1):
    """Kalman, constant sensor, local mode, 200 x 200 at 0.1 m: handles to elevation, variance, _kalman_p and a user
    layer held across every device operation."""
    rng = np.random.default_rng(seed)
    s = MS.Script("handles")
    s.op("map", "A", 20, 20, 0.1, 0, 0, 0)
    s.op("fastdem", "M", "A")
    s.op("estimator", "M", "kalman")
    s.op("sensor", "M", "constant", 0.04)
    s.op("mode", "M", "local")
    s.op("height", "M", -3, 3)
    s.op("range", "M", 0, 30)
    s.pose("TBS", MS.yaw_pose(0.1, 0.0, 0.6))
    path = [(0.3 * k * np.cos(0.4 * k), 0.3 * k * np.sin(0.4 * k)) for k in range(80)]
    k = [0]

    def nxt(n=4000, name=None):
        i = k[0]
        k[0] += 1
        x, y = path[i % len(path)]
        T = MS.yaw_pose(x, y, 0.0, 0.2 * i)
        s.pose(f"P{i}", T)
        c = name or f"c{i}"
        s.cloud(c, *MS.scan(rng, n, T @ s.poses["TBS"], centre=(x, y)))
        return c, f"P{i}", (x, y)

    s.op("add", "A", "user", 0.5)
    c, p, _ = nxt()
    s.op("integrate", "M", c, "TBS", p)
    s.op("touch", "A", "elevation")
    for h, layer in (("hE", "elevation"), ("hV", "variance"), ("hK", "_kalman_p"), ("hU", "user")):
        s.op("get", h, "A", layer)
    s.op("dump", "A")
    handles = lambda: [("hE", rng.uniform(-0.5, 0.5)), ("hK", rng.uniform(1e-4, 5e-3)), ("hV", 0.003),
                       ("hU", rng.uniform(0, 1))]
    empty = "cempty"
    s.cloud(empty, np.zeros(0), np.zeros(0), np.zeros(0))
    xy = path[1]
    _touch_and_write(s, "A", handles(), rng, xy)
    # every entry point in turn, each followed by a host access, handle writes and a dump
    kinds = ["integrate", "integrate4", "batch1", "batch16", "batch17", "batch33", "cloud2", "queued", "mapmove",
             "inpaint", "inpaint_inplace", "smooth", "smooth_obstacle", "fusion", "features", "raycasting", "clear",
             "clearat", "hfill", "hdata", "addm", "integrate"]
    for kind in kinds:
        if kind == "integrate" or kind == "integrate4":
            c, p, _ = nxt()
            s.op(kind, "M", c, "TBS", p)
        elif kind.startswith("batch"):
            n = int(kind[5:])
            items = []
            for j in range(n):
                if n > 1 and j == n // 2:
                    items.append(f"{empty}:TBS:P0")
                else:
                    c, p, _ = nxt(600)
                    items.append(f"{c}:TBS:{p}")
            s.op("batch", "M", *items)
        elif kind == "cloud2":
            c, p, _ = nxt(3000)
            cl = s.clouds[c]
            n = cl["x"].size
            rec = np.zeros((n, 8), dtype=np.float32)     # x y z pad intensity pad pad pad (Velodyne-like, 32 bytes)
            rec[:, 0], rec[:, 1], rec[:, 2] = cl["x"], cl["y"], cl["z"]
            rec[:, 4] = rng.uniform(0, 100, n)
            rec[::97, 1] = np.nan                        # (non-finite points are dropped by from_impl)
            s.blobs["msg.bin"] = rec.tobytes()
            s.op("cloud2", "M", "msg.bin", n, 32, "x:0:7,y:4:7,z:8:7,intensity:16:7,ring:20:4", "TBS", p)
        elif kind == "queued":
            s.op("queued", "M", 1)
            c, p, _ = nxt()
            s.op("integrate", "M", c, "TBS", p)
            s.op("integrate", "M", empty, "TBS", p)
            c, p, _ = nxt()
            s.op("integrate", "M", c, "TBS", p)
            s.op("drain", "M")
            s.op("queued", "M", 0)
        elif kind == "mapmove":
            s.op("mapmove", "A", MS._g(xy[0] + 3.73), MS._g(xy[1] - 2.41))    # strips that wrap
        elif kind == "inpaint":
            s.op("inpaint", "A", 3, 2, 0)
        elif kind == "inpaint_inplace":
            s.op("inpaint", "A", 2, 2, 1)
        elif kind == "smooth":
            s.op("smooth", "A", "elevation", 3, 5)
        elif kind == "smooth_obstacle":
            s.op("smooth", "A", "obstacle", 3, 4)
        elif kind == "fusion":
            s.op("fusion", "A", 0.15, 0.05, 0.01, 0.99, 3)
        elif kind == "features":
            s.op("features", "A", 0.3, 4, 0.05, 0.95)
        elif kind == "raycasting":
            c, p, (x, y) = nxt(3000)
            T = s.poses[p] @ s.poses["TBS"]
            P = T @ np.stack([s.clouds[c]["x"], s.clouds[c]["y"], s.clouds[c]["z"], np.ones(s.clouds[c]["x"].size)])
            s.cloud(c + "w", P[0], P[1], P[2])       # (applyRaycasting takes the scan in the map frame)
            s.op("raycasting", "A", c + "w", MS._g(T[0, 3]), MS._g(T[1, 3]), MS._g(T[2, 3]))
        elif kind == "clear":
            s.op("clear", "A", "user")
        elif kind == "clearat":
            s.op("touch", "A", "elevation")
            s.op("clearat", "A", int(rng.integers(0, 200)), int(rng.integers(0, 200)))
        elif kind == "hfill":
            s.op("touch", "A", "elevation")
            s.op("hfill", "hU", 0.25)
            c, p, _ = nxt()
            s.op("integrate", "M", c, "TBS", p)
        elif kind == "hdata":
            s.op("touch", "A", "elevation")
            s.op("hdata", "hU", int(rng.integers(0, 40000)), 0.75)
            s.op("mapmove", "A", MS._g(xy[0] - 1.05), MS._g(xy[1] + 0.55))
        elif kind == "addm":
            s.blobs["user2.f32"] = rng.uniform(-1, 1, 40000).astype(np.float32).tobytes()
            s.op("addm", "A", "user2", "user2.f32")
            s.op("add", "A", "user", 0.125)                 # (add on an existing layer)
        xy = path[k[0] % len(path)]
        _touch_and_write(s, "A", handles(), rng, xy)
    return s


def script_forks(seed=2):
    """Copy construction, copy assignment, std::move construction, move assignment and snapshot() mid-stream, with a
    handle written but not yet flushed, or the host copies stale after an integrate; then both sides go on with
    mappers of their own.  ElevationMapping::update on a map of its own."""
    rng = np.random.default_rng(seed)
    s = MS.Script("forks")
    s.pose("TBS", MS.yaw_pose(0.0, 0.0, 0.5))
    s.op("map", "S", 16, 16, 0.1, 0.4, -0.3, 0)
    s.op("fastdem", "MS", "S")
    s.op("sensor", "MS", "lidar", 0.03, 0.002)
    s.op("height", "MS", -2, 2)
    n = [0]

    def scan(mapper, centre, pts=3000):
        i = n[0]
        n[0] += 1
        T = MS.yaw_pose(centre[0], centre[1], 0.0, 0.3 * i)
        s.pose(f"P{i}", T)
        s.cloud(f"c{i}", *MS.scan(rng, pts, T @ s.poses["TBS"], radius=5.0, centre=centre, lift=0.05 * i))
        s.op("integrate", mapper, f"c{i}", "TBS", f"P{i}")

    for j in range(3):
        scan("MS", (0.2 * j, 0.1 * j))
    s.op("touch", "S", "elevation")
    s.op("get", "hS", "S", "elevation")
    s.op("get", "hSK", "S", "_kalman_p")
    s.op("dump", "S")

    def pending(slot, h):           # a host access, then a write through the held handle that has not been flushed
        s.op("touch", slot, "variance")
        s.op("hwritepos", h, MS._g(rng.uniform(-1, 1)), MS._g(rng.uniform(-1, 1)), MS._g(rng.uniform(0.5, 1.5)))
        s.op("at", slot, "variance", int(rng.integers(0, 160)), int(rng.integers(0, 160)), 0.004)

    # copy construction with a pending write
    pending("S", "hS")
    s.op("copy", "C", "S")
    s.op("dump", "C")
    s.op("fastdem", "MC", "C")
    s.op("sensor", "MC", "constant", 0.05)
    s.op("queued", "MC", 1)
    scan("MS", (0.5, 0.0))
    scan("MC", (-0.5, 0.4))
    s.op("drain", "MC")
    s.op("dump", "S")
    s.op("dump", "C")
    # copy assignment into C, whose queued mapper stays bound, with a pending write on S
    pending("S", "hS")
    s.op("copyassign", "C", "S")
    s.op("dump", "C")
    scan("MC", (0.0, -0.6))
    scan("MS", (0.6, 0.6))
    s.op("drain", "MC")
    s.op("dump", "S")
    s.op("dump", "C")
    # std::move construction of a map whose host copies are stale, with a write pending before the scan
    pending("S", "hS")
    scan("MS", (0.3, 0.3))
    s.op("move", "D", "S")
    s.op("dump", "D")                   # (held handles hS / hSK now read D)
    s.op("fastdem", "MD", "D")
    s.op("sensor", "MD", "lidar", 0.03, 0.002)
    scan("MD", (0.1, -0.2))
    s.op("dump", "D")
    # move assignment: a fresh copy of D scanned, stale, then moved over C
    s.op("copy", "S2", "D")
    s.op("fastdem", "MS2", "S2")
    scan("MS2", (-0.4, -0.4))
    s.op("touch", "S2", "elevation")
    s.op("get", "h2", "S2", "elevation")
    s.op("hwritepos", "h2", 0.0, 0.0, 2.5)
    scan("MS2", (-0.2, -0.4))
    s.op("moveassign", "C", "S2")
    s.op("dump", "C")
    s.op("fastdem", "MC2", "C")
    scan("MC2", (0.2, 0.5))
    scan("MD", (0.4, -0.1))
    s.op("dump", "C")
    s.op("dump", "D")
    # snapshot with a pending write
    pending("D", "hS")
    s.op("snapshot", "N", "D", "elevation,variance,_kalman_p")
    s.op("dump", "N")
    s.op("fastdem", "MN", "N")
    scan("MN", (0.0, 0.2))
    scan("MD", (0.1, 0.1))
    s.op("dump", "N")
    s.op("dump", "D")
    # ElevationMapping on a map of its own
    s.op("map", "E", 12, 12, 0.1, 0, 0, 0)
    s.op("emapping", "ME", "E", "local", "kalman")
    for j in range(3):
        T = MS.yaw_pose(0.2 * j, 0.0, 0.5)
        x, y, z = MS.scan(rng, 2000, np.eye(4), radius=4.0, centre=(0.2 * j, 0.0))
        s.cloud(f"u{j}", x, y, z)
        s.op("update", "ME", f"u{j}", MS._g(0.2 * j), 0.0)
        s.op("touch", "E", "elevation")
        if j == 0:
            s.op("get", "hEE", "E", "elevation")
        s.op("hwrite", "hEE", 60, 60 + j, 0.7)
        s.op("dump", "E")
    return s


def script_p2(seed=3):
    """P2 with colour and intensity: the RGB-D sensor, global mode and FastDEM(map, loadConfig(default.yaml)) —
    raycasting on; writes through held _p2_q* / _p2_n* handles between scans, queued scans behind them."""
    rng = np.random.default_rng(seed)
    s = MS.Script("p2")
    s.op("map", "G", 14, 12, 0.1, 1.0, -0.5, 0)
    s.op("fastdem", "MP", "G", "default.yaml")
    s.op("sensor", "MP", "type", "rgbd")
    s.op("mode", "MP", "global")
    s.op("estimator", "MP", "p2")
    T_bs = MS.yaw_pose(0.0, 0.0, 1.2)
    T_bs[:3, :3] = [[1, 0, 0], [0, -1, 0], [0, 0, -1]]    # (looking down: positive depth for the RGB-D model)
    s.pose("TBS", T_bs)
    hs = ["_p2_q0", "_p2_q2", "_p2_q4", "_p2_n1", "_p2_n3"]
    for i in range(9):
        T = MS.yaw_pose(1.0 + 0.2 * np.cos(i), -0.5 + 0.2 * np.sin(i), 0.0, 0.1 * i)
        s.pose(f"P{i}", T)
        x, y, z = MS.scan(rng, 2500, T @ T_bs, radius=4.0, centre=(T[0, 3], T[1, 3]))
        inten = rng.uniform(0, 255, x.size).astype(np.float32)
        rgb = rng.integers(0, 1 << 24, x.size).astype(np.uint32)
        s.cloud(f"c{i}", x, y, z, intensity=inten, rgb=rgb)
        if i == 4:
            s.op("queued", "MP", 1)
        s.op("integrate", "MP", f"c{i}", "TBS", f"P{i}")
        if i >= 4:
            continue                                      # (queued: no host access until the drain)
        s.op("touch", "G", "elevation")
        if i == 0:
            for j, ln in enumerate(hs):
                s.op("get", f"h{j}", "G", ln)
        for j, ln in enumerate(hs):
            v = rng.uniform(-0.2, 0.4) if "_q" in ln else float(rng.integers(1, 6))
            s.op("hwritepos", f"h{j}", MS._g(1.0 + rng.uniform(-1, 1)), MS._g(-0.5 + rng.uniform(-1, 1)), MS._g(v))
        s.op("dump", "G")
    s.op("drain", "MP")
    s.op("touch", "G", "elevation")
    s.op("dump", "G")
    return s


def script_move_clear_basic(seed=4):
    """move_clear_basic on: user layers and held handles across moves shorter than the map and beyond it."""
    rng = np.random.default_rng(seed)
    s = MS.Script("move_clear_basic")
    s.op("map", "B", 10, 10, 0.1, 0, 0, 1)
    s.op("setstart", "B", 17, 42)
    s.op("setpos", "B", 0.05, -0.05)
    s.op("fastdem", "MB", "B")
    s.op("sensor", "MB", "constant", 0.03)
    s.op("mode", "MB", "global")
    s.pose("TBS", MS.yaw_pose(0.0, 0.0, 0.5))
    s.op("add", "B", "u1", 1.5)
    s.op("add", "B", "u2")
    centre = np.zeros(2)
    for i, step in enumerate([(0.0, 0.0), (2.35, -1.15), (0.0, 3.05), (13.3, 2.2), (-4.45, -4.45), (25.0, -31.0)]):
        if i:
            centre = centre + np.asarray(step)
            s.op("mapmove", "B", MS._g(centre[0]), MS._g(centre[1]))
            s.op("touch", "B", "u1")
            s.op("dump", "B")
        T = MS.yaw_pose(centre[0], centre[1], 0.0, 0.5 * i)
        s.pose(f"P{i}", T)
        s.cloud(f"c{i}", *MS.scan(rng, 3000, T @ s.poses["TBS"], radius=4.0, centre=tuple(centre)))
        s.op("integrate", "MB", f"c{i}", "TBS", f"P{i}")
        s.op("touch", "B", "u1")
        if i == 0:
            s.op("get", "hu1", "B", "u1")
            s.op("get", "hu2", "B", "u2")
            s.op("get", "hel", "B", "elevation")
        for h in ("hu1", "hu2", "hel"):
            s.op("hwrite", h, int(rng.integers(0, 100)), int(rng.integers(0, 100)), MS._g(rng.uniform(-1, 1)))
        s.op("hwritepos", "hel", MS._g(centre[0] + 0.2), MS._g(centre[1]), 0.9)
        s.op("atpos", "B", "u2", MS._g(centre[0] - 0.3), MS._g(centre[1] + 0.1), 3.0)
        s.op("dump", "B")
    s.op("clearall", "B")
    s.op("touch", "B", "u1")
    s.op("dump", "B")
    s.op("integrate", "MB", "c0", "TBS", "P0")
    s.op("touch", "B", "u1")
    s.op("dump", "B")
    return s


def script_host_sensor(seed=5):
    """A user SensorModel subclass returning the built-in LiDAR model's covariance (σ_z² evaluated on the host) against
    the oracle's built-in LiDAR; both scan callbacks recorded."""
    rng = np.random.default_rng(seed)
    s = MS.Script("host_sensor")
    s.op("map", "H", 12, 12, 0.1, 0, 0, 0)
    s.op("fastdem", "MH", "H")
    s.op("sensor", "MH", "hostlidar", 0.025, 0.0015)
    s.op("height", "MH", -1.5, 1.5)
    s.op("range", "MH", 0.3, 9.0)
    s.op("callbacks", "MH", 1)
    s.op("raycast", "MH", 1)
    T_bs = MS.yaw_pose(0.05, -0.02, 0.7, 0.3)
    c, sn = np.cos(0.2), np.sin(0.2)
    T_bs[:3, :3] = T_bs[:3, :3] @ np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]])   # (pitched: R is not a yaw)
    s.pose("TBS", T_bs)
    for i in range(6):
        T = MS.yaw_pose(0.3 * i, -0.1 * i, 0.02 * i, 0.4 * i)
        s.pose(f"P{i}", T)
        s.cloud(f"c{i}", *MS.scan(rng, 2500, T @ T_bs, radius=6.0, centre=(0.3 * i, -0.1 * i)))
    s.op("integrate", "MH", "c0", "TBS", "P0")
    s.op("integrate4", "MH", "c1", "TBS", "P1")
    s.op("batch", "MH", "c2:TBS:P2", "c3:TBS:P3")
    s.op("touch", "H", "elevation")
    s.op("dump", "H")
    s.op("queued", "MH", 1)                               # (a user sensor model keeps integrate() synchronous)
    s.op("integrate", "MH", "c4", "TBS", "P4")
    s.op("callbacks", "MH", 0)
    s.op("sensor", "MH", "lidar", 0.025, 0.0015)
    s.op("integrate", "MH", "c5", "TBS", "P5")
    s.op("drain", "MH")
    s.op("touch", "H", "elevation")
    s.op("dump", "H")
    return s


def script_large(seed=6):
    """Scans of 220 K points (the large-scan pipeline and its held-back update) meeting the mirror's uploads: handle
    writes between queued scans."""
    rng = np.random.default_rng(seed)
    s = MS.Script("large")
    s.op("map", "L", 24, 24, 0.1, 0, 0, 0)
    s.op("fastdem", "ML", "L")
    s.op("sensor", "ML", "lidar", 0.02, 0.001)
    s.op("height", "ML", -2, 2)
    s.pose("TBS", MS.yaw_pose(0.0, 0.0, 0.8))
    for i in range(4):
        T = MS.yaw_pose(0.5 * i, 0.25 * i, 0.0, 0.15 * i)
        s.pose(f"P{i}", T)
        s.cloud(f"c{i}", *MS.scan(rng, 220_000, T @ s.poses["TBS"], radius=10.0, centre=(0.5 * i, 0.25 * i)))
    s.op("integrate", "ML", "c0", "TBS", "P0")
    s.op("touch", "L", "elevation")
    s.op("get", "hE", "L", "elevation")
    s.op("get", "hK", "L", "_kalman_p")
    s.op("dump", "L")
    s.op("queued", "ML", 1)
    for i in (1, 2, 3):
        s.op("touch", "L", "elevation")
        s.op("hwritepos", "hE", MS._g(0.5 * i + 0.1), MS._g(0.25 * i), MS._g(0.3 * i))
        s.op("hwritepos", "hK", MS._g(0.5 * i - 0.2), MS._g(0.25 * i + 0.1), 0.0005)
        s.op("integrate", "ML", f"c{i}", "TBS", f"P{i}")
        if i == 2:
            s.op("drain", "ML")
    s.op("drain", "ML")
    s.op("touch", "L", "elevation")
    s.op("dump", "L")
    return s


SCRIPTS = (script_handles, script_forks, script_p2, script_move_clear_basic, script_host_sensor, script_large)
_cache = {}


def _oracle(R, make):
    if make not in _cache:
        s = make()
        o = MS.OracleReplay(R, yaml_dir=os.path.dirname(YAML))
        R.set_trig_mode(1)      # (correctly rounded trig, as the device evaluates it: feature extraction bit for bit)
        try:
            o.run(s)
        finally:
            R.set_trig_mode(0)
        _cache[make] = (s, o)
    return _cache[make]


# -------------------------------------------------------------------------------------------------- CPU checks ----
def test_scripts_are_deterministic():
    for make in SCRIPTS:
        a, b = make(), make()
        assert a.lines == b.lines and a.blobs == b.blobs, make.__name__


def test_every_step_kind_occurs():
    ops = {t[0] for make in SCRIPTS for t in make().steps()}
    need = {"map", "setpos", "setstart", "copy", "copyassign", "move", "moveassign", "snapshot", "fastdem", "emapping",
            "estimator", "sensor", "height", "range", "mode", "queued", "callbacks", "integrate", "integrate4", "batch",
            "cloud2", "drain", "update", "touch", "get", "hwrite", "hwritepos", "hfill", "hdata", "at", "atpos",
            "clearat", "add", "addm", "clear", "mapmove", "inpaint", "smooth", "fusion", "features", "raycasting",
            "dump", "setpos", "setstart", "clearall", "raycast"}
    missing = need - ops
    assert not missing, missing


@pytest.mark.parametrize("make", SCRIPTS, ids=lambda f: f.__name__[7:])
def test_oracle_side_runs_and_is_not_vacuous(R, make):
    s, o = _oracle(R, make)
    dumps = [r for r in o.records if r[0] == "dump"]
    assert dumps, s.name
    assert any(np.isfinite(r[4]["elevation"]).sum() > 100 for r in dumps), s.name
    name = s.name
    if name in ("handles", "large", "move_clear_basic", "p2"):
        assert o.observed > 0, f"{name}: no handle write lands in a cell a later scan observes"
    if name in ("handles", "move_clear_basic"):
        assert o.moves > 0, f"{name}: no move shifted the map"
    if name == "forks":
        assert {f[0] for f in o.forks} == set(MS.FORK_OPS)
        # the source and destination of every fork diverge once both have scanned on their own
        last = {}
        for r in dumps:
            last[r[2]] = r[4]["elevation"]
        for a, b in (("C", "D"), ("N", "D")):
            assert not np.array_equal(last[a], last[b], equal_nan=True), (a, b)
    if name == "p2":
        assert all(np.isfinite(dumps[-1][4][f"_p2_q{i}"]).sum() > 100 for i in range(5))
        assert "raycasting" in dumps[-1][4] or "_visibility_logodds" in dumps[-1][4], sorted(dumps[-1][4])
    if name == "host_sensor":
        cbs = [r for r in o.records if r[0] == "cb"]
        assert {r[1] for r in cbs} == {"pre", "ras"} and all(r[2][0].size > 0 for r in cbs)
    if name == "large":
        assert max(c["x"].size for c in s.clouds.values()) >= 200_000


def test_replay_without_gpu_fails_loudly(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    if not os.path.exists(BINS["ndebug"]):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fastdem_amd", "cpp")])
    s = MS.Script("nogpu")
    s.op("map", "A", 4, 4, 0.1, 0, 0, 0)
    s.op("dump", "A")
    s.write(str(tmp_path))
    for b in BINS.values():
        r = subprocess.run([b, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no HIP device" in (r.stdout + r.stderr), r.stdout + r.stderr


# -------------------------------------------------------------------------------------------------- GPU checks ----
@pytest.mark.gpu
@pytest.mark.parametrize("make", SCRIPTS, ids=lambda f: f.__name__[7:])
def test_mirror_matches_oracle(gpu, R, make, tmp_path):
    """Both builds of the replay binary, one process at a time.  A run that exits non-zero fails the test at once and
    starts nothing more; a run that differs from the oracle is reported together with the other build's result."""
    s, o = _oracle(R, make)
    opts = [f"option {k} {int(v)}" for k, v in sorted(gpu.Engine.default_options.items())]
    errors = []
    for flavour, exe in BINS.items():
        assert os.access(exe, os.X_OK), f"{exe} is not built (make -C fastdem_amd/cpp)"
        d = str(tmp_path / flavour)
        run = MS.Script(s.name)
        run.lines, run.blobs = opts + s.lines, s.blobs
        run.write(d, FILES)
        r = subprocess.run([exe, d], capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert r.returncode == 0, "\n".join(errors + [
            f"{s.name} ({flavour}): exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"])
        got = MS.read_replay(d)
        assert got[-1] == ("end", len(run.lines)), got[-1]
        try:
            MS.compare(f"{s.name} ({flavour})", _shift(got, len(opts)), o.records, s.steps())
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, "\n".join(errors)


def _shift(recs, k):
    """Step numbers of the binary (option lines first) -> step numbers of the script."""
    out = []
    for r in recs:
        if r[0] in ("ret", "dump"):
            r = (r[0], r[1] - k) + tuple(r[2:])
        out.append(r)
    return out
