"""Scripts for the C++ host mirror (fastdem_amd/cpp/include) and their oracle side.

A script is a list of text steps (the format fastdem_amd/cpp/tests/mirror_replay.cpp reads) plus the binary inputs
they name.  `Script.write(dir)` lays it out for the replay binary; `OracleReplay(R).run(script)` performs the same
steps on fdm_ref_py maps; `read_replay(dir)` reads what the binary wrote.  Both sides yield the same records:
  ("ret", step, op, value, stats-or-None)   every returned bool (+ lastStats())
  ("dump", step, slot, info, layers, handles) the map of a slot: every layer and every live handle
  ("cb", kind, arrays)                       a scan-callback cloud
"""
import os

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)

# fastdem::Config{} as the C++ mirror default-constructs it (fdm_config field names)
CPP_DEFAULTS = dict(
    z_min=-FLT_MAX, z_max=FLT_MAX, range_min=0.0, range_max=FLT_MAX, sensor_type=1,
    lidar_range_noise=0.02, lidar_angular_noise=0.001, rgbd_normal_a=0.001, rgbd_normal_b=0.002,
    rgbd_normal_c=0.4, rgbd_lateral_factor=0.001, constant_uncertainty=0.03, mode=0, estimation_type=0,
    kalman_min_variance=0.0001, kalman_max_variance=0.01, kalman_process_noise=0.0,
    p2_dn=(0.01, 0.16, 0.50, 0.84, 0.99), p2_elevation_marker=3, p2_max_sample_count=0.0, raycast_enabled=0,
    rc_height_conflict_threshold=0.05, rc_log_odds_observed=0.4, rc_log_odds_ghost=0.2, rc_log_odds_max=2.0,
    rc_clear_threshold=-1.0)

SCAN_OPS = ("integrate", "integrate4", "batch", "cloud2", "update")
FORK_OPS = ("copy", "copyassign", "move", "moveassign", "snapshot")


def _g(v):
    return repr(float(v))


class Script:
    def __init__(self, name):
        self.name = name
        self.lines = []
        self.blobs = {}
        self.clouds = {}     # name -> dict(x, y, z, intensity, rgb)
        self.poses = {}      # name -> 4x4 float64

    def op(self, *tok):
        self.lines.append(" ".join(str(t) for t in tok))

    def pose(self, name, T):
        T = np.asarray(T, dtype=np.float64)
        self.poses[name] = T
        self.op("pose", name, *(_g(v) for v in T.reshape(16)))

    def cloud(self, name, x, y, z, intensity=None, rgb=None):
        x, y, z = (np.ascontiguousarray(v, dtype=np.float32) for v in (x, y, z))
        self.clouds[name] = dict(x=x, y=y, z=z, intensity=intensity, rgb=rgb)
        if x.size:
            self.blobs[name + ".xyz.f32"] = np.concatenate([x, y, z]).tobytes()
        if intensity is not None:
            self.blobs[name + ".i.f32"] = np.ascontiguousarray(intensity, dtype=np.float32).tobytes()
        if rgb is not None:
            self.blobs[name + ".rgb.u32"] = np.ascontiguousarray(rgb, dtype=np.uint32).tobytes()
        self.op("cloud", name, x.size, int(intensity is not None), int(rgb is not None))

    def steps(self):
        return [ln.split() for ln in self.lines]

    def write(self, d, files=None):
        os.makedirs(os.path.join(d, "out"), exist_ok=True)
        with open(os.path.join(d, "script.txt"), "w") as f:
            f.write("\n".join(self.lines) + "\n")
        for k, v in self.blobs.items():
            with open(os.path.join(d, k), "wb") as f:
                f.write(v)
        for k, src in (files or {}).items():
            with open(src, "rb") as a, open(os.path.join(d, k), "wb") as b:
                b.write(a.read())


# ------------------------------------------------------------------------------------------------ scene helpers ----
def yaw_pose(x, y, z=0.0, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = (x, y, z)
    return T


def terrain(x, y):
    return (0.15 * np.sin(0.7 * x) + 0.1 * np.cos(0.9 * y) + 0.3 * ((np.abs(x - 2.0) < 0.6) & (np.abs(y + 1.0) < 0.6))
            ).astype(np.float64)


def scan(rng, n, T_ws, radius=6.0, centre=(0.0, 0.0), noise=0.01, lift=0.0):
    """n points of the terrain around `centre` (world frame), handed over in the sensor frame of T_ws."""
    r = radius * np.sqrt(rng.random(n))
    a = rng.random(n) * 2 * np.pi
    wx, wy = centre[0] + r * np.cos(a), centre[1] + r * np.sin(a)
    wz = terrain(wx, wy) + noise * rng.standard_normal(n) + lift
    obst = rng.random(n) < 0.05                           # some tall returns (obstacles, ghosts for raycasting)
    wz = np.where(obst, wz + 0.8 * rng.random(n), wz)
    P = np.stack([wx, wy, wz, np.ones(n)])
    S = np.linalg.inv(T_ws) @ P
    return S[0].astype(np.float32), S[1].astype(np.float32), S[2].astype(np.float32)


# ------------------------------------------------------------------------------------------------------ oracle ----
class _Mapper:
    def __init__(self, slot, cfg, sensor):
        self.slot, self.cfg, self.sensor = slot, dict(cfg), sensor
        self.queued = False
        self.callbacks = False
        self.pending = None      # (rc, stats) of the last queued scan, until drain()
        self.stats = None


def _cfg_from_struct(c):
    out = {}
    for k in CPP_DEFAULTS:
        v = getattr(c, k)
        out[k] = tuple(v[i] for i in range(5)) if k == "p2_dn" else v
    return out


def _sensor_of(cfg):
    """createSensorModel(cfg.sensor_model)."""
    t = cfg["sensor_type"]
    if t == 0:
        return ("constant", cfg["constant_uncertainty"])
    if t == 2:
        return ("rgbd", cfg["rgbd_normal_a"], cfg["rgbd_normal_b"], cfg["rgbd_normal_c"], cfg["rgbd_lateral_factor"])
    return ("lidar", cfg["lidar_range_noise"], cfg["lidar_angular_noise"])


class OracleReplay:
    """The script on fdm_ref_py maps: a copy or snapshot is a fresh oracle map with the same geometry, start index and
    layers; a move hands the slot over; a handle write is a set_layer of that cell (visible at once, as a write through
    a reference is in the reference)."""

    def __init__(self, R, yaml_dir=None):
        self.R = R
        self.yaml_dir = yaml_dir
        self.maps, self.mcb, self.mappers, self.handles = {}, {}, {}, {}
        # a map no mapper has been bound to yet holds the ElevationMap's basic layers and what was added to it; an
        # oracle map always carries its estimator's layers as well, which a dump leaves out until a mapper binds
        self.bare = {}
        self.records = []
        self.writes = []        # (step, slot, layer, (r, c), value): handle / at() writes, for the coverage checks
        self.watch = []         # writes waiting for the next scan of their map: (slot, (r, c), n_points then)
        self.observed = 0       # writes whose cell the next scan of the map observed
        self.forks = []         # (op, destination, source)
        self.moves = 0          # mapmove steps that shifted the map

    # -- helpers --
    def _ref_cfg(self, d):
        c = self.R.default_config()
        for k, v in d.items():
            if k == "p2_dn":
                for i in range(5):
                    c.p2_dn[i] = v[i]
            else:
                setattr(c, k, v)
        return c

    def _effective(self, m):
        d = dict(m.cfg)
        s = m.sensor
        if s[0] == "constant":
            d.update(sensor_type=0, constant_uncertainty=s[1])
        elif s[0] in ("lidar", "hostlidar"):   # (the host-side subclass returns the LiDAR model's covariance)
            d.update(sensor_type=1, lidar_range_noise=abs(s[1]), lidar_angular_noise=abs(s[2]))
        elif s[0] == "rgbd":
            d.update(sensor_type=2, rgbd_normal_a=s[1], rgbd_normal_b=s[2], rgbd_normal_c=s[3],
                     rgbd_lateral_factor=s[4])
        return d

    def _fork(self, src, layers=None):
        g = src.geometry()
        ref = self.R.RefEngine(np.float32(g.length_x), np.float32(g.length_y), np.float32(g.resolution),
                               position=(g.position_x, g.position_y))
        ref.set_start_index(g.start_row, g.start_col)
        for name in (layers if layers is not None else src.layers()):
            if not src.exists(name):
                continue
            if not ref.exists(name):
                ref.add(name)
            ref.set_layer(name, src.layer(name))
        return ref

    def _write_cell(self, step, slot, layer, rc, value):
        ref = self.maps[slot]
        a = ref.layer(layer)
        a[rc] = np.float32(value)
        ref.set_layer(layer, a)
        self.writes.append((step, slot, layer, rc, np.float32(value)))
        if ref.exists("n_points"):
            self.watch.append((slot, rc, ref.layer("n_points")[rc]))

    def _scanned(self, slot):
        keep = []
        for s, rc, n in self.watch:
            if s != slot:
                keep.append((s, rc, n))
                continue
            now = self.maps[slot].layer("n_points")[rc] if slot in self.maps and self.maps[slot].exists("n_points") else n
            self.observed += int(not np.array_equal(now, n, equal_nan=True))
        self.watch = keep

    def _drop_mappers(self, slot):
        for k in [k for k, m in self.mappers.items() if m.slot == slot]:
            del self.mappers[k]

    def _drop_handles(self, slot):
        for k in [k for k, h in self.handles.items() if h[0] == slot]:
            del self.handles[k]

    def _scan(self, m, c, tbs, twb):
        """integrate(cloud, T_base_sensor, T_world_base) on the mapper's map; (bool, stats) as the mirror returns."""
        cl = self.clouds[c]
        if cl["x"].size == 0:
            return False, m.stats
        ref = self.maps[m.slot]
        ref.set_config(self._ref_cfg(self._effective(m)))
        ref.capture(m.callbacks)
        rc, st = ref.integrate(cl["x"], cl["y"], cl["z"], self.poses[tbs], self.poses[twb],
                               intensity=cl["intensity"], rgb=cl["rgb"])
        m.stats = st
        if rc == 0 and m.callbacks:
            self._callbacks(ref, st)
        return rc == 0, st

    def _callbacks(self, ref, st):
        x, y, z, _ = ref.last_preprocessed(st["n_input"])
        cov = ref.last_preprocessed_cov(st["n_input"]).transpose(0, 2, 1).reshape(-1)
        self.records.append(("cb", "pre", [x, y, z, cov]))
        if st["n_cells_touched"] > 0:
            self.records.append(("cb", "ras", list(ref.last_rasterized(st["n_cells_touched"]))))

    # -- the interpreter --
    def run(self, script):
        self.clouds, self.poses = script.clouds, script.poses
        self.script = script
        for step, t in enumerate(script.steps()):
            try:
                self.exec(step, t)
            except Exception as e:
                raise RuntimeError(f"{script.name}: oracle step {step} ({' '.join(t)}): {e!r}") from e
        return self.records

    def exec(self, step, t):
        op, a = t[0], t[1:]
        R = self.R
        self._exec(step, op, a, R)
        if op in SCAN_OPS:
            slot = self.mappers[a[0]].slot
            self._scanned(slot)
        if op in FORK_OPS:
            self.forks.append((op, a[0], a[1]))
        if op == "mapmove" and self.records[-1][3]:
            self.moves += 1

    def _exec(self, step, op, a, R):
        if op in ("option", "pose", "cloud"):
            return
        if op == "map":
            self._drop_mappers(a[0])
            self._drop_handles(a[0])
            ref = R.RefEngine(float(a[1]), float(a[2]), float(a[3]), position=(float(a[4]), float(a[5])))
            ref.set_move_clear_basic(bool(int(a[6])))
            self.maps[a[0]], self.mcb[a[0]] = ref, bool(int(a[6]))
            self.bare[a[0]] = {"elevation", "elevation_min", "elevation_max"}
        elif op == "setpos":
            self.maps[a[0]].set_position(float(a[1]), float(a[2]))
        elif op == "setstart":
            self.maps[a[0]].set_start_index(int(a[1]), int(a[2]))
        elif op in ("copy", "copyassign"):
            ref = self._fork(self.maps[a[1]])
            ref.set_move_clear_basic(self.mcb[a[1]])
            if op == "copy":
                self._drop_mappers(a[0])
            self._drop_handles(a[0])
            self.maps[a[0]], self.mcb[a[0]] = ref, self.mcb[a[1]]
            self.bare.pop(a[0], None)
        elif op in ("move", "moveassign"):
            self._drop_mappers(a[0])
            self._drop_handles(a[0])
            self._drop_mappers(a[1])
            self.maps[a[0]] = self.maps.pop(a[1])
            self.mcb[a[0]] = self.mcb.pop(a[1])
            self.bare.pop(a[0], None)
            if a[1] in self.bare:
                self.bare[a[0]] = self.bare.pop(a[1])
            for k, h in list(self.handles.items()):
                if h[0] == a[1]:
                    self.handles[k] = (a[0], h[1])
        elif op == "snapshot":
            self._drop_mappers(a[0])
            self._drop_handles(a[0])
            self.maps[a[0]] = self._fork(self.maps[a[1]], layers=a[2].split(","))
            self.mcb[a[0]] = False
            self.bare[a[0]] = {"elevation", "elevation_min", "elevation_max"} | set(a[2].split(","))
        elif op == "drop":
            self._drop_mappers(a[0])
            self._drop_handles(a[0])
            del self.maps[a[0]]
        elif op == "fastdem":
            if len(a) > 2:
                from fastdem_amd.config import load_config
                cfg = _cfg_from_struct(load_config(os.path.join(self.yaml_dir, a[2])))
            else:
                cfg = dict(CPP_DEFAULTS)
            self.mappers[a[0]] = _Mapper(a[1], cfg, _sensor_of(cfg))
            self.bare.pop(a[1], None)
        elif op == "emapping":
            cfg = dict(CPP_DEFAULTS, mode=int(a[2] == "global"), estimation_type=int(a[3] == "p2"))
            self.mappers[a[0]] = _Mapper(a[1], cfg, _sensor_of(cfg))
            self.bare.pop(a[1], None)
            self.maps[a[1]].set_config(self._ref_cfg(cfg))
        elif op == "estimator":
            self.mappers[a[0]].cfg["estimation_type"] = int(a[1] == "p2")
        elif op == "sensor":
            m = self.mappers[a[0]]
            if a[1] == "type":
                m.cfg["sensor_type"] = {"constant": 0, "lidar": 1, "rgbd": 2}[a[2]]
                m.sensor = _sensor_of(m.cfg)
            else:
                m.sensor = (a[1],) + tuple(float(np.float32(v)) for v in a[2:])
        elif op == "height":
            self.mappers[a[0]].cfg.update(z_min=float(a[1]), z_max=float(a[2]))
        elif op == "range":
            self.mappers[a[0]].cfg.update(range_min=float(a[1]), range_max=float(a[2]))
        elif op == "mode":
            self.mappers[a[0]].cfg["mode"] = int(a[1] == "global")
        elif op == "raycast":
            self.mappers[a[0]].cfg["raycast_enabled"] = int(a[1])
        elif op == "queued":
            m = self.mappers[a[0]]
            if not int(a[1]):
                self._drain(m)
            m.queued = bool(int(a[1]))
        elif op == "callbacks":
            self.mappers[a[0]].callbacks = bool(int(a[1]))
        elif op == "integrate":
            m = self.mappers[a[0]]
            queued = m.queued and not m.callbacks and m.sensor[0] != "hostlidar"
            if queued:
                if self.clouds[a[1]]["x"].size == 0:
                    self.records.append(("ret", step, op, False, None))
                    return
                ok, st = self._scan(m, *a[1:4])
                m.pending = (ok, st)
                self.records.append(("ret", step, op, True, None))
            else:
                self._drain(m)
                ok, st = self._scan(m, *a[1:4])
                self.records.append(("ret", step, op, ok, None if m.queued else st))
        elif op == "integrate4":
            m = self.mappers[a[0]]
            self._drain(m)
            ok, st = self._scan(m, *a[1:4])
            self.records.append(("ret", step, op, ok, st))
        elif op == "batch":
            m = self.mappers[a[0]]
            self._drain(m)
            last = False
            for s in a[1:]:
                c, tb, tw = s.split(":")
                last, _ = self._scan(m, c, tb, tw)
            self.records.append(("ret", step, op, last, m.stats))
        elif op == "cloud2":
            m = self.mappers[a[0]]
            self._drain(m)
            ref = self.maps[m.slot]
            lay = R.RefCloud2Layout(point_step=int(a[3]), off_x=-1, off_y=-1, off_z=-1, off_intensity=-1,
                                    intensity_type=0, off_rgb=-1)
            for fld in a[4].split(","):                       # FieldOffsets::parse (impl.hpp:65-99)
                name, off, dt = fld.split(":")
                if name in ("x", "y", "z"):
                    setattr(lay, "off_" + name, int(off))
                elif name == "intensity":
                    lay.off_intensity, lay.intensity_type = int(off), int(dt)
                elif name in ("rgb", "rgba"):
                    lay.off_rgb = int(off)
            ref.set_config(self._ref_cfg(self._effective(m)))
            ref.capture(m.callbacks)
            rc, st = ref.integrate_cloud2(self.script.blobs[a[1]], int(a[2]), lay, self.poses[a[5]], self.poses[a[6]])
            m.stats = st
            self.records.append(("ret", step, op, rc == 0, st))
        elif op == "drain":
            m = self.mappers[a[0]]
            ok = self._drain(m)
            self.records.append(("ret", step, op, ok, m.stats))
        elif op == "update":
            m = self.mappers[a[0]]
            cl = self.clouds[a[1]]
            ref = self.maps[m.slot]
            st = ref.update(cl["x"], cl["y"], cl["z"], robot_xy=(float(a[2]), float(a[3])),
                            intensity=cl["intensity"], rgb=cl["rgb"])
            self.records.append(("ret", step, "update", True, (st["n_cells_touched"], st["n_in_map"])))
        elif op == "touch":
            return
        elif op == "get":
            if not self.maps[a[1]].exists(a[2]):
                raise KeyError(a[2])
            self.handles[a[0]] = (a[1], a[2])
        elif op == "hwrite":
            slot, layer = self.handles[a[0]]
            self._write_cell(step, slot, layer, (int(a[1]), int(a[2])), float(a[3]))
        elif op == "hwritepos":
            slot, layer = self.handles[a[0]]
            ok, rc = self.maps[slot].get_index(float(a[1]), float(a[2]))
            assert ok, "hwritepos outside the map"
            self._write_cell(step, slot, layer, rc, float(a[3]))
        elif op == "hfill":
            slot, layer = self.handles[a[0]]
            ref = self.maps[slot]
            ref.set_layer(layer, np.full((ref.rows, ref.cols), np.float32(float(a[1])), dtype=np.float32))
        elif op == "hdata":
            slot, layer = self.handles[a[0]]
            k = int(a[1])
            self._write_cell(step, slot, layer, (k % self.maps[slot].rows, k // self.maps[slot].rows), float(a[2]))
        elif op == "at":
            self._write_cell(step, a[0], a[1], (int(a[2]), int(a[3])), float(a[4]))
        elif op == "atpos":
            ok, rc = self.maps[a[0]].get_index(float(a[2]), float(a[3]))
            assert ok, "atpos outside the map"
            self._write_cell(step, a[0], a[1], rc, float(a[4]))
        elif op == "clearat":
            ref = self.maps[a[0]]
            for name in ref.layers():
                self._write_cell(step, a[0], name, (int(a[1]), int(a[2])), float("nan"))
        elif op == "add":
            self.maps[a[0]].add(a[1], float(a[2]) if len(a) > 2 else float("nan"))
            if a[0] in self.bare:
                self.bare[a[0]].add(a[1])
        elif op == "addm":
            ref = self.maps[a[0]]
            arr = np.frombuffer(self.script.blobs[a[2]], dtype=np.float32).reshape(ref.cols, ref.rows).T
            if not ref.exists(a[1]):
                ref.add(a[1])
            ref.set_layer(a[1], arr)
            if a[0] in self.bare:
                self.bare[a[0]].add(a[1])
        elif op == "clear":
            self.maps[a[0]].clear(a[1])
        elif op == "clearall":
            self.maps[a[0]].clear(None)
        elif op == "mapmove":
            ref = self.maps[a[0]]
            g0 = ref.geometry()
            ref.move(float(a[1]), float(a[2]))
            g1 = ref.geometry()
            self.records.append(("ret", step, op, (g0.start_row, g0.start_col) != (g1.start_row, g1.start_col), None))
        elif op == "inpaint":
            self.maps[a[0]].apply_inpainting(int(a[1]), int(a[2]), bool(int(a[3])))
        elif op == "smooth":
            if self.maps[a[0]].exists(a[1]):
                self.maps[a[0]].apply_spatial_smoothing(a[1], int(a[2]), int(a[3]))
        elif op == "fusion":
            ref = self.maps[a[0]]
            if ref.exists("upper_bound") and ref.exists("lower_bound"):
                ref.apply_uncertainty_fusion(True, float(np.float32(a[1])), float(np.float32(a[2])),
                                             float(np.float32(a[3])), float(np.float32(a[4])), int(a[5]))
        elif op == "features":
            if self.maps[a[0]].exists("elevation"):
                self.maps[a[0]].apply_feature_extraction(float(np.float32(a[1])), int(a[2]), float(np.float32(a[3])),
                                                         float(np.float32(a[4])))
        elif op == "raycasting":
            cl = self.clouds[a[1]]
            if cl["x"].size:            # (the wrapper hands over config::Raycasting{} with enabled = true)
                ref = self.maps[a[0]]
                saved = R.config_from(ref.cfg)
                c = R.config_from(ref.cfg)
                for k in ("raycast_enabled", "rc_height_conflict_threshold", "rc_log_odds_observed",
                          "rc_log_odds_ghost", "rc_log_odds_max", "rc_clear_threshold"):
                    setattr(c, k, 1 if k == "raycast_enabled" else CPP_DEFAULTS[k])
                ref.set_config(c)
                ref.apply_raycasting(cl["x"], cl["y"], cl["z"], np.array([float(v) for v in a[2:5]], dtype=np.float32))
                ref.set_config(saved)
        elif op == "dump":
            ref = self.maps[a[0]]
            g = ref.geometry()
            info = (g.rows, g.cols, g.start_row, g.start_col, g.position_x, g.position_y)
            layers = {n: ref.layer(n) for n in ref.layers() if a[0] not in self.bare or n in self.bare[a[0]]}
            handles = {k: (h[1], ref.layer(h[1])) for k, h in self.handles.items() if h[0] == a[0]}
            self.records.append(("dump", step, a[0], info, layers, handles))
        else:
            raise ValueError(f"unknown op {op}")

    def _drain(self, m):
        if m.pending is None:
            return True
        ok, _ = m.pending
        m.pending = None
        return ok


# ------------------------------------------------------------------------------------------------ the C++ side ----
def read_replay(d):
    """The records the replay binary wrote under d/out (the same shapes as OracleReplay's)."""
    out = os.path.join(d, "out")
    recs = []
    lines = open(os.path.join(out, "log.txt")).read().splitlines()
    i = 0
    while i < len(lines):
        t = lines[i].split()
        if t[0] == "ret":
            step, op, v = int(t[1]), t[2], bool(int(t[3]))
            if op == "update":
                st = (int(t[4]), int(t[5]))
            elif len(t) > 4:
                st = dict(zip(("n_input", "n_after_filter", "n_in_map", "n_cells_touched", "shift_rows",
                               "shift_cols"), (int(x) for x in t[4:10])))
            else:
                st = None
            recs.append(("ret", step, op, v, st))
        elif t[0] == "cb":
            k, kind, n, has_cov = int(t[1]), t[2], int(t[3]), int(t[4])
            raw = np.fromfile(os.path.join(out, f"cb_{k}.f32"), dtype=np.float32)
            arrs = [raw[:n], raw[n:2 * n], raw[2 * n:3 * n]]
            if has_cov:
                arrs.append(raw[3 * n:])
            recs.append(("cb", kind, arrs))
        elif t[0] == "dump":
            step, k, slot = int(t[1]), int(t[2]), t[3]
            rows, cols, sr, sc = (int(x) for x in t[4:8])
            info = (rows, cols, sr, sc, float(t[8]), float(t[9]))
            raw = np.fromfile(os.path.join(out, f"dump_{k}.f32"), dtype=np.float32)
            layers, handles, off = {}, {}, 0
            i += 1
            while lines[i] != "enddump":
                u = lines[i].split()
                arr = raw[off:off + rows * cols].reshape(cols, rows).T
                off += rows * cols
                if u[0] == "layer":
                    layers[u[1]] = arr
                else:
                    handles[u[1]] = (u[2], arr)
                i += 1
            recs.append(("dump", step, slot, info, layers, handles))
        elif t[0] == "end":
            recs.append(("end", int(t[1])))
        i += 1
    return recs


# ------------------------------------------------------------------------------------------------- comparison ----
def _first_diff(a, b):
    """Index of the first cell whose bits differ (NaN equal to NaN, signed zeros distinguished), or None."""
    na, nb = np.isnan(a), np.isnan(b)
    ia, ib = a.view(np.uint32), b.view(np.uint32)
    bad = (na != nb) | (~na & ~nb & (ia != ib))
    if not bad.any():
        return None
    r, c = np.argwhere(bad)[0]
    return int(r), int(c), int(bad.sum())


def compare(name, got, want, steps):
    """Every record bit for bit; the message names the script, the step and the first differing cell."""
    got = [r for r in got if r[0] != "end"]

    def where(step):
        return f"{name}: step {step} ({' '.join(steps[step])})"

    assert len(got) == len(want), f"{name}: {len(got)} records from the mirror, {len(want)} from the oracle"
    for g, w in zip(got, want):
        assert g[0] == w[0], f"{name}: record kinds differ: {g[:3]} vs {w[:3]}"
        if g[0] == "ret":
            assert g[1:4] == w[1:4], f"{where(w[1])}: returned {g[3]}, the oracle {w[3]}"
            if w[4] is not None or g[4] is not None:
                assert g[4] == w[4], f"{where(w[1])}: stats {g[4]} vs the oracle's {w[4]}"
        elif g[0] == "cb":
            assert g[1] == w[1], f"{name}: callback kinds differ {g[1]} vs {w[1]}"
            if g[1] == "pre":   # in order, covariances included
                for k, (a, b) in enumerate(zip(g[2], w[2])):
                    assert a.shape == b.shape and a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes(), \
                        f"{name}: preprocessed cloud channel {k} differs ({a.size} vs {b.size} values)"
            else:               # as a set (the order of the cells is the engine's)
                ka = sorted(zip(*(v.view(np.uint32).tolist() for v in g[2][:3])))
                kb = sorted(zip(*(v.view(np.uint32).tolist() for v in w[2][:3])))
                assert ka == kb, f"{name}: rasterized clouds differ ({len(ka)} vs {len(kb)} points)"
        else:
            _, step, slot, info, layers, handles = g
            assert (step, slot) == (w[1], w[2]), f"{name}: dumps out of step: {(step, slot)} vs {w[1:3]}"
            assert info == w[3], f"{where(step)}: map '{slot}' geometry (rows, cols, start, position) {info} vs {w[3]}"
            assert sorted(layers) == sorted(w[4]), f"{where(step)}: layers {sorted(layers)} vs {sorted(w[4])}"
            for ln in sorted(w[4]):
                d = _first_diff(layers[ln], w[4][ln])
                assert d is None, (f"{where(step)}: map '{slot}' layer '{ln}' differs in {d[2]} cells, first at "
                                   f"({d[0]}, {d[1]}): {layers[ln][d[:2]]!r} vs the oracle's {w[4][ln][d[:2]]!r}")
            assert sorted(handles) == sorted(w[5]), f"{where(step)}: handles {sorted(handles)} vs {sorted(w[5])}"
            for h in sorted(w[5]):
                layer, arr = handles[h]
                assert layer == w[5][h][0], f"{where(step)}: handle '{h}' is of layer '{layer}', not '{w[5][h][0]}'"
                for other, what in ((w[5][h][1], "the oracle's layer"), (layers[layer], "a fresh get()")):
                    d = _first_diff(arr, other)
                    assert d is None, (f"{where(step)}: map '{slot}' handle '{h}' ({layer}) differs from {what} in "
                                       f"{d[2]} cells, first at ({d[0]}, {d[1]}): {arr[d[:2]]!r} vs {other[d[:2]]!r}")
