"""k_pcd_decode (fastdem_amd/csrc/fdm_pcd.hpp) behind fdm_pcd_decode against the restatement of loadPCD's binary branch
and readFieldAsFloat (tests/pcd_restate.py), bit for bit: record sizes on both sides of every path the kernel takes
(LDS staging up to 128 bytes with 16-, 4- and 1-byte loads by the body's alignment, the direct path above), point counts
around the 256-point block, the conversions' edge values, and the refusals.  The kernel has no chunk or grid boundary
besides the block: a launch takes up to 2^32 - 1 points in blocks of 256.

Run on the GPU box:  python -m pytest tests -m gpu
"""
import struct

import numpy as np
import pytest

import pcd_cases as PC
import pcd_gpu_util as U
import pcd_restate as PR

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1000]


def file_of(point_size, n, seed=0):
    fields = PC.LAYOUTS[point_size]
    return PC.layout_header(fields, n), PC.random_records(fields, n, seed + point_size)


@pytest.mark.parametrize("point_size", [s for s in sorted(PC.LAYOUTS) if s != 1025])
def test_every_layout(gpu, point_size):
    header, body = file_of(point_size, 257)
    want = U.restated(header, body)
    assert PR.parse_header(header).point_size == point_size
    for placement in ("pageable", "device+0", "device+1", "device+4"):
        U.assert_same(U.decode(gpu, header, body, placement), want, placement)
    U.assert_same(U.decode(gpu, header, body, "device+3", device=0), want, "device outputs")


@pytest.mark.parametrize("n", COUNTS)
def test_every_count_and_placement(gpu, n):
    for point_size in (12, 13):                       # the minimal layout, and the smallest with an odd record size
        header, body = file_of(point_size, n, seed=n)
        want = U.restated(header, body)
        for placement in U.PLACEMENTS:
            U.assert_same(U.decode(gpu, header, body, placement), want, f"{point_size} {placement}")
        U.assert_same(U.decode(gpu, header, body + b"trailing bytes", "pinned", device=0), want, "device outputs")


@pytest.mark.parametrize("point_size", [16, 19, 32, 48, 128, 129, 257])
def test_unaligned_device_bodies(gpu, point_size):
    header, body = file_of(point_size, 300, seed=7)
    want = U.restated(header, body)
    for placement in U.PLACEMENTS[2:]:              # pinned memory from inside the block, device memory
        U.assert_same(U.decode(gpu, header, body, placement), want, placement)


def test_conversion_edge_values(gpu):
    header, body = PC.special_values()
    want = U.restated(header, body)
    # the restatement's own answers for the cases named in the issue, so that a wrong restatement cannot agree with a
    # wrong kernel unnoticed
    x = want["x"]
    assert x[3] == F32(2.0 ** -127) and x[3] != 0                  # rounds to a float subnormal
    assert x[4].view(np.uint32) == 1 and x[5].view(np.uint32) == 0      # 1e-45 -> the smallest subnormal, 7e-46 -> 0
    assert x[6].view(np.uint32) == 0                                    # 2^-150, half of the smallest subnormal: to even
    assert np.isinf(x[7]) and x[7] > 0 and np.isinf(x[8]) and x[8] < 0 and np.isinf(x[9])   # beyond FLT_MAX + half an ulp
    assert x[10] == F32(1.0) and x[11].view(np.uint32) == 0x3F800001 and x[12].view(np.uint32) == 0x3F800002   # ties to even
    assert want["intensity"][3] == F32(16777216.0) and want["intensity"][4] == F32(16777220.0)
    assert want["intensity"][6] == F32(4294967296.0) and want["intensity"][7] == F32(4294967040.0)
    assert want["nx"][2] == F32(-2147483648.0)
    assert want["y"][0].view(np.uint32) == 0x7FC00001 and want["y"][1].view(np.uint32) == 0xFFC12345    # payloads kept
    assert (want["rgb"] >> 24 == 0).all() and want["rgb"][1] == 0x010203
    for placement in ("pageable", "device+0", "device+1"):
        got = U.decode(gpu, header, body, placement)
        U.assert_same(got, want, placement)
        assert got["y"].tobytes() == want["y"].tobytes() and got["nz"].tobytes() == want["nz"].tobytes()   # F4: bits, NaN too


@pytest.mark.parametrize("type_,size", PC.UNSUPPORTED)
def test_unsupported_pairs_read_as_zero(gpu, type_, size):
    fields = PC.unsupported_layout(type_, size)
    header, body = PC.layout_header(fields, 70), PC.random_records(fields, 70, 11)
    want = U.restated(header, body)
    assert not want["x"].any() and not want["intensity"].any() and want["y"].any()
    for placement in ("pageable", "device+1"):
        U.assert_same(U.decode(gpu, header, body, placement), want, placement)


def test_no_point_is_dropped(gpu):
    bits = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0x3F800000, 0xFFFFFFFF], dtype=np.uint32)
    rec = np.stack([bits, np.roll(bits, 1), np.roll(bits, 2)], 1)
    header, body = PC.layout_header(PC.LAYOUTS[12], 5), rec.tobytes()
    got = U.decode(gpu, header, body)
    assert got["x"].view(np.uint32).tolist() == bits.tolist() and got["z"].view(np.uint32).tolist() == np.roll(bits, 2).tolist()


def refused(gpu, header, body, placement="pageable"):
    with pytest.raises(PR.PcdError):
        U.restated(header, body)
    with pytest.raises(gpu.EngineError):
        U.decode(gpu, header, body, placement)
    return gpu.capi.load().fdm_last_error().decode()


def test_refusals(gpu):
    header, body = file_of(1025, 3)
    assert "1024" in refused(gpu, header, body)
    header, body = file_of(19, 100)
    assert "end of binary data" in refused(gpu, header, body[:-1])                  # a short body
    assert "end of binary data" in refused(gpu, header, body[:-1], "device+1")
    colour_at_end = PC.xyz_f4([("rgb", "U", 1, 1)])                                 # its 4 bytes would leave the record
    assert "colour" in refused(gpu, PC.layout_header(colour_at_end, 2), bytes(26))
    assert "point size of 0" in refused(gpu, b"FIELDS x y z\nSIZE 0 0 0\nWIDTH 2\nDATA binary\n", b"")
    count0 = [("x", "F", 4, 1), ("y", "F", 4, 1), ("pad", "U", 1, 2), ("z", "F", 4, 0)]   # z: no bytes of its own
    assert "beyond the record" in refused(gpu, PC.layout_header(count0, 2), bytes(20))
    assert "x, y, z" in refused(gpu, b"FIELDS x y\nWIDTH 1\nDATA binary\n", bytes(8))


def test_empty_cloud_and_absent_channels(gpu):
    got = U.decode(gpu, PC.layout_header(PC.LAYOUTS[16], 0), b"")
    assert got["x"].size == 0 and got["intensity"] is None
    header, body = file_of(48, 10)
    got = U.decode(gpu, header, body)
    assert got["intensity"] is None and got["rgb"] is not None and got["nx"] is not None


def test_load_pcd_fixture(gpu):
    import os
    want = PR.three_points()
    for name in ("three_points_binary.pcd", "three_points_ascii.pcd"):
        for device in (None, 0):
            c = gpu.pcd.load_pcd(os.path.join(PR.GOLDEN, name), device=device)
            if device is not None:
                c = {k: None if v is None else v.cpu().numpy().view(np.uint32 if k == "rgb" else F32) for k, v in c.items()}
            U.assert_same(c, want, name)
