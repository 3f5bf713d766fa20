"""FastDEM::setVoxelAnyOrder through the C++ host mirror, end to end: fastdem_amd/cpp/tests/voxel_order_npz.cpp builds a
LOCAL raycasting map from VLP-16 scans with the mirror's public API and writes it to .npz; the oracle runs the same scans
with the matching voxel order.  Half-way the map is replaced by a copy of itself (a new engine), so the mapper has to
set the option on that engine too."""
import os
import struct
import subprocess

import numpy as np
import pytest

from mirror_script import CPP_DEFAULTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fastdem_amd", "cpp", "build", "fdm_voxel_order_npz")
N_SCANS, FORK_AT = 6, 3


def ref_cfg(R):
    c = R.default_config()
    d = dict(CPP_DEFAULTS, mode=0, z_min=-2.0, z_max=4.0, range_min=0.2, range_max=14.0, raycast_enabled=1)
    for k, v in d.items():
        if k == "p2_dn":
            for i in range(5):
                c.p2_dn[i] = v[i]
        else:
            setattr(c, k, v)
    return c


def fork(R, src):
    """What copy assignment leaves: a fresh map with the same geometry, start index and layers."""
    g = src.geometry()
    ref = R.RefEngine(np.float32(g.length_x), np.float32(g.length_y), np.float32(g.resolution),
                      position=(g.position_x, g.position_y))
    ref.set_start_index(g.start_row, g.start_col)
    for name in src.layers():
        if not ref.exists(name):
            ref.add(name)
        ref.set_layer(name, src.layer(name))
    return ref


def oracle(R, wl, poses, stable):
    ref = R.RefEngine(24.0, 24.0, 0.1)
    for k in range(N_SCANS):
        if k == FORK_AT:
            ref = fork(R, ref)
        ref.set_voxel_stable(stable)
        ref.set_config(ref_cfg(R))
        s = wl.scan(k)
        ref.integrate(s["x"], s["y"], s["z"], wl.T_base_sensor, poses[k], intensity=s["intensity"])
    return ref


def run_mirror(tmp_path, wl, poses, order):
    d = tmp_path / order
    d.mkdir()
    with open(d / "scans.bin", "wb") as f:
        f.write(struct.pack("<II", N_SCANS, FORK_AT))
        f.write(np.asarray(wl.T_base_sensor, dtype=np.float64).tobytes())
        for k in range(N_SCANS):
            s = wl.scan(k)
            f.write(struct.pack("<I", s["x"].size))
            for c in ("x", "y", "z", "intensity"):
                f.write(np.ascontiguousarray(s[c], dtype=np.float32).tobytes())
            f.write(np.asarray(poses[k], dtype=np.float64).tobytes())
    r = subprocess.run([BIN, str(d), order], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return dict(np.load(d / "out.npz"))


def same_map(out, ref):
    g = ref.geometry()
    if tuple(out["_geometry"]) != (g.rows, g.cols, g.start_row, g.start_col):
        return False
    names = sorted(k for k in out if k != "_geometry")
    if names != sorted(ref.layers()):
        return False
    for n in names:
        a, b = out[n], ref.layer(n)
        na, nb = np.isnan(a), np.isnan(b)
        if not np.array_equal(na, nb) or not np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)):
            return False
    return True


def test_mirror_voxel_any_order_against_the_oracle(gpu, R, tmp_path):
    assert os.path.exists(BIN), "build() makes fastdem_amd/cpp/build/fdm_voxel_order_npz"
    wl = gpu.synth.vlp16(n_scans=N_SCANS)
    poses = [wl.pose(k) for k in range(N_SCANS)]
    lit, stb = oracle(R, wl, poses, stable=False), oracle(R, wl, poses, stable=True)
    assert lit.exists("raycasting")
    assert not same_map({**{n: lit.layer(n) for n in lit.layers()},
                         "_geometry": np.array([lit.geometry().rows, lit.geometry().cols, lit.geometry().start_row,
                                                lit.geometry().start_col])}, stb), \
        "the scans have no teeth: std::sort's order and the stable order give the same map"
    out = run_mirror(tmp_path, wl, poses, "stdsort")
    assert same_map(out, lit), "setVoxelAnyOrder(StdSort) differs from the oracle's std::sort order"
    assert not same_map(out, stb)
    out = run_mirror(tmp_path, wl, poses, "stable")
    assert same_map(out, stb), "the stable order differs from the oracle's stable order"
