"""The pcd2dem pipeline from a file: fdm_pcd_build_dem must give, bit for bit, what fdm_engine_build_dem gives on the arrays
the restatement of loadPCD (tests/pcd_restate.py) decodes from the same file — geometry, stage counts and every layer;
fdm_engine_to_pcd must give the restatement's savePCD records of fdm_engine_to_point_cloud's arrays.  The cloud is the
1 400-point shape of tests/test_build_dem_gpu.py, written as a binary PCD with 19-byte records and as ASCII.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import functools

import numpy as np
import pytest

import pcd_cases as PC
import pcd_restate as PR
from helpers import assert_layers_bit_identical, same_geometry
from test_build_dem_gpu import CONFIG, dem_cloud

pytestmark = pytest.mark.gpu
F32 = np.float32


@functools.lru_cache(maxsize=None)
def dem_file(channels, fmt):
    """(file bytes, the restatement's decode of them)."""
    c = dem_cloud()
    n = c["x"].size
    xyz = np.stack([c["x"], c["y"], c["z"]], 1).astype("<f4").view(np.uint8).reshape(n, 12)
    rng = np.random.default_rng(9)
    if channels:          # x y z | rgb U4 | intensity U1 | two bytes of padding = 19
        fields = PC.xyz_f4([("rgb", "U", 4, 1), ("intensity", "U", 1, 1), ("_", "U", 1, 2)])
        rec = np.concatenate([xyz, c["rgb"].astype("<u4").view(np.uint8).reshape(n, 4),
                              np.round(c["intensity"] * 255).astype(np.uint8).reshape(n, 1),
                              rng.integers(0, 256, (n, 2), dtype=np.uint8)], 1)
    else:                 # x y z | ring U2 | time F4 | flag U1 = 19
        fields = PC.xyz_f4([("ring", "U", 2, 1), ("time", "F", 4, 1), ("flag", "U", 1, 1)])
        rec = np.concatenate([xyz, rng.integers(0, 256, (n, 7), dtype=np.uint8)], 1)
    assert rec.shape[1] == 19
    data = PC.layout_header(fields, n) + rec.tobytes()
    h, cloud = PR.load(data)
    assert h.point_size == 19 and cloud["x"].tobytes() == c["x"].tobytes()
    if fmt == "ascii":    # the same cloud through savePCD's ASCII branch: eight decimals
        data = PR.save(cloud, PR.ASCII)
        h, cloud = PR.load(data)
        assert h.format == PR.ASCII and h.point_size == (20 if channels else 12)
    assert (cloud["intensity"] is not None) == channels and (cloud["rgb"] is not None) == channels
    for v in cloud.values():
        if v is not None:
            v.setflags(write=False)
    return data, cloud


@pytest.mark.parametrize("method", ["max", "mean"])
@pytest.mark.parametrize("channels", [False, True])
@pytest.mark.parametrize("inpaint", [0, 3])
def test_pcd_build_dem(gpu, method, channels, inpaint):
    cfg = gpu.DEMConfig(method=method, inpaint_iterations=inpaint, **CONFIG)
    for fmt in ("binary", "ascii"):
        data, cloud = dem_file(channels, fmt)
        ref, st = gpu.build_dem(cloud["x"], cloud["y"], cloud["z"], cloud["intensity"], cloud["rgb"], config=cfg,
                                return_stats=True)
        eng, rc = gpu.pcd.build_dem(data, cfg, return_stats=True)
        assert ref is not None and eng is not None and rc == st["status"] == 0
        assert st["n_after_height"] < st["n_after_sor"] < st["n_input"] == cloud["x"].size
        assert same_geometry(eng.geometry(), ref.geometry())
        assert eng.layers() == ref.layers() and ("intensity" in eng.layers()) == channels
        assert_layers_bit_identical(eng, ref)
        assert np.isfinite(eng.layer("elevation")).sum() > 100
        # ... and the way out: savePCD(toPointCloud(map))'s records
        c = eng.to_point_cloud()
        body, n, hi, hc = eng.to_pcd()
        assert n == c["x"].size and hi == (c["intensity"] is not None) == channels and hc == (c["rgb"] is not None)
        assert body == PR.save_body(c, PR.BINARY)
        eng.close()
        ref.close()


def test_to_pcd_into_a_small_buffer(gpu):
    import ctypes as C
    data, cloud = dem_file(True, "binary")
    eng = gpu.pcd.build_dem(data, gpu.DEMConfig(**CONFIG))
    body, n, hi, hc = eng.to_pcd()
    buf = np.full(len(body), 0xAA, dtype=np.uint8)
    nb, npts = C.c_uint64(0), C.c_uint64(0)
    lib = gpu.capi.load()
    rc = lib.fdm_engine_to_pcd(eng._h, buf.ctypes.data_as(C.c_void_p), len(body) - 1, C.byref(nb), C.byref(npts), None, None)
    assert rc == gpu.capi.FDM_SKIP_BUFFER_TOO_SMALL and nb.value == len(body) and npts.value == n and (buf == 0xAA).all()
    rc = lib.fdm_engine_to_pcd(eng._h, buf.ctypes.data_as(C.c_void_p), len(body), C.byref(nb), C.byref(npts), None, None)
    assert rc == 0 and buf.tobytes() == body
    eng.close()


@pytest.mark.parametrize("fmt", ["binary", "ascii"])
def test_pcd2dem_writes_the_file(gpu, tmp_path, fmt):
    data, cloud = dem_file(True, fmt)
    src, dst = str(tmp_path / "in.pcd"), str(tmp_path / "out.pcd")
    with open(src, "wb") as f:
        f.write(data)
    cfg = gpu.DEMConfig(**CONFIG)
    ref = gpu.build_dem(cloud["x"], cloud["y"], cloud["z"], cloud["intensity"], cloud["rgb"], config=cfg)
    want = ref.to_point_cloud()
    ref.close()
    n = gpu.pcd.pcd2dem(src, dst, cfg)
    assert n == want["x"].size > 100
    with open(dst, "rb") as f:
        assert f.read() == PR.save(want, PR.BINARY)
    back = gpu.pcd.load_pcd(dst)
    for k in ("x", "y", "z", "intensity", "rgb"):
        assert back[k].tobytes() == want[k].tobytes(), k
    assert back["nx"] is None


def test_files_without_a_map(gpu, tmp_path):
    empty = PC.layout_header(PC.LAYOUTS[16], 0)
    eng, rc = gpu.pcd.build_dem(empty, return_stats=True)
    assert eng is None and rc == gpu.capi.FDM_SKIP_EMPTY_CLOUD
    one = PC.layout_header(PC.LAYOUTS[12], 1) + np.ones(3, "<f4").tobytes()
    eng, rc = gpu.pcd.build_dem(one, return_stats=True)
    assert eng is None and rc == gpu.capi.FDM_SKIP_ALL_FILTERED
    data, _ = dem_file(False, "binary")
    eng, rc = gpu.pcd.build_dem(data, gpu.DEMConfig(sor_k=0), return_stats=True)
    assert eng is None and rc == gpu.capi.FDM_SKIP_ALL_FILTERED
    src, dst = str(tmp_path / "in.pcd"), str(tmp_path / "out.pcd")
    with open(src, "wb") as f:
        f.write(empty)
    assert gpu.pcd.pcd2dem(src, dst) == 0                 # a file of 0 points, as the tool writes it
    with open(dst, "rb") as f:
        assert f.read() == PR.save_header(0, False, False, False)


def test_refusals(gpu):
    data, _ = dem_file(False, "binary")
    h = PR.parse_header(data)
    body = bytearray(data[h.data_offset:])
    body[19 * 5 + 8:19 * 5 + 12] = np.array([np.nan], "<f4").tobytes()          # z of the sixth point
    with pytest.raises(gpu.EngineError, match="not finite"):
        gpu.pcd.build_dem(data[:h.data_offset] + bytes(body))
    with pytest.raises(gpu.EngineError, match="end of binary data"):
        gpu.pcd.build_dem(data[:-1])
    with pytest.raises(gpu.EngineError):
        gpu.pcd.build_dem(data, gpu.DEMConfig(sor_k=65))
