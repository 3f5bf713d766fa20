"""k_pcd_pack (fastdem_amd/csrc/fdm_pcd.hpp) behind fdm_pcd_encode: the binary data section equals the bytes the
restatement of savePCD writes (tests/pcd_restate.py), for every channel subset, around the 256-point block, from host
and from device arrays; and decode(encode(cloud)) is the cloud.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import ctypes as C

import numpy as np
import pytest

import pcd_gpu_util as U
import pcd_restate as PR

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1000]
SUBSETS = {"none": (), "intensity": ("intensity",), "rgb": ("rgb",), "normals": ("nx", "ny", "nz"),
           "all": ("intensity", "rgb", "nx", "ny", "nz")}


def cloud(n, channels, seed):
    """Random bit patterns in every float channel (NaN payloads, infinities, subnormals), colours with a top byte."""
    rng = np.random.default_rng(seed)
    c = {k: None for k in U.CHANNELS}
    for k in ("x", "y", "z") + tuple(channels):
        bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        c[k] = bits if k == "rgb" else bits.view(F32)
    return c


@pytest.mark.parametrize("subset", sorted(SUBSETS))
@pytest.mark.parametrize("n", COUNTS)
def test_binary_encode(gpu, subset, n):
    import torch
    c = cloud(n, SUBSETS[subset], n)
    want = PR.save_body(c, PR.BINARY)
    assert len(want) == n * (12 + 4 * len(SUBSETS[subset]))
    assert gpu.pcd.encode(c) == want
    d = {k: None if v is None else torch.from_numpy(v.view(np.int32)).cuda() for k, v in c.items()}
    d = {k: None if v is None else (v if k == "rgb" else v.view(torch.float32)) for k, v in d.items()}
    assert gpu.pcd.encode(d) == want
    # decode(encode(c)) == c, the colour's top byte aside
    header = PR.save_header(n, c["intensity"] is not None, c["rgb"] is not None, c["nx"] is not None)
    back = U.decode(gpu, header, want, "device+0")
    for k in U.CHANNELS:
        assert (back[k] is None) == (c[k] is None)
        if c[k] is not None:
            assert back[k].tobytes() == (c[k] & np.uint32(0xFFFFFF) if k == "rgb" else c[k]).tobytes(), k


def test_a_buffer_one_byte_short(gpu):
    lib = gpu.capi.load()
    c = cloud(300, ("intensity",), 1)
    want = PR.save_body(c, PR.BINARY)
    p = [c[k].ctypes.data_as(C.c_void_p) for k in ("x", "y", "z", "intensity")]
    buf = np.full(len(want), 0xAA, dtype=np.uint8)
    need = C.c_uint64(0)
    args = (300, *p, None, None, None, None, 0, 1, 8, 0, buf.ctypes.data_as(C.c_void_p))
    assert lib.fdm_pcd_encode(*args, len(want) - 1, C.byref(need)) == gpu.capi.FDM_SKIP_BUFFER_TOO_SMALL
    assert need.value == len(want) and (buf == 0xAA).all()
    assert lib.fdm_pcd_encode(*args, len(want), C.byref(need)) == 0 and buf.tobytes() == want


def test_refusals_and_the_empty_cloud(gpu):
    lib = gpu.capi.load()
    c = cloud(4, ("nx", "ny"), 2)
    with pytest.raises(gpu.EngineError):
        gpu.pcd.encode(c)                                   # two of the three normal arrays
    assert gpu.pcd.encode(cloud(0, ("intensity",), 3)) == b""
    need = C.c_uint64(9)
    assert lib.fdm_pcd_encode(4, None, None, None, None, None, None, None, None, 0, 1, 8, 0, None, 0, C.byref(need)) == \
        gpu.capi.FDM_ERR_INVALID


def test_save_pcd_writes_the_restatements_file(gpu, tmp_path):
    c = cloud(257, SUBSETS["all"], 5)
    path = str(tmp_path / "b.pcd")
    vp = (1.0, 2.0, 3.0, 0.5, 0.5, 0.5, 0.5)
    gpu.pcd.save_pcd(path, c, viewpoint=vp)
    with open(path, "rb") as f:
        assert f.read() == PR.save(c, PR.BINARY, viewpoint=vp)
    back, h = gpu.pcd.load_pcd(path, return_header=True)
    assert tuple(h.viewpoint) == vp and back["nz"].tobytes() == c["nz"].tobytes()
