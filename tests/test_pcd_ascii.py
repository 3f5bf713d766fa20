"""ASCII PCD records through the C ABI — fdm_pcd_decode into host arrays, fdm_pcd_encode from host arrays — against the
restatement of loadPCD's and savePCD's ASCII branches (tests/pcd_restate.py).  Host code only: no device is touched.
Colour tokens are decimal integers; what std::stoul makes of other text is not restated."""
import numpy as np
import pytest

import pcd_cases as PC
import pcd_restate as PR

F32 = np.float32


@pytest.fixture(scope="module")
def pcd():
    from fastdem_amd import pcd
    return pcd


def bits(u):
    return np.asarray(u, dtype=np.uint32).view(F32)


def edge_values():
    """NaN of both signs and with a payload, infinities, zeros of both signs, subnormals, the largest float, values whose
    eighth decimal rounds up, and ordinary ones."""
    v = bits([0x7FC00000, 0xFFC00000, 0x7F812345, 0x7F800000, 0xFF800000, 0, 0x80000000, 1, 0x80000001, 0x007FFFFF,
              0x7F7FFFFF, 0xFF7FFFFF, 0x00800000])
    rng = np.random.default_rng(3)
    return np.concatenate([v, F32([0.1, -0.1, 0.999999995, 1.0000000049, 123456.789, -9.9999999e-9, 0.0005, 0.0015, 2.5e-9]),
                           rng.normal(0, 100, 40).astype(F32), (rng.normal(0, 1, 40) * 1e-6).astype(F32)])


def edge_cloud(channels):
    v = edge_values()
    n = v.size
    c = {"x": v, "y": np.roll(v, 1), "z": np.roll(v, 2), "intensity": None, "rgb": None, "nx": None, "ny": None, "nz": None}
    if "intensity" in channels:
        c["intensity"] = np.roll(v, 3)
    if "rgb" in channels:
        c["rgb"] = (np.arange(n, dtype=np.uint64) * 2654435761 % 2 ** 24).astype(np.uint32)
        c["rgb"][:3] = [0, 0xFFFFFF, 0x010203]
    if "normals" in channels:
        c["nx"], c["ny"], c["nz"] = np.roll(v, 4), np.roll(v, 5), np.roll(v, 6)
    return c


SUBSETS = [(), ("intensity",), ("rgb",), ("normals",), ("intensity", "rgb", "normals")]


@pytest.mark.parametrize("channels", SUBSETS)
@pytest.mark.parametrize("precision", [8, 3, 0])
def test_ascii_encode(pcd, channels, precision):
    c = edge_cloud(channels)
    want = PR.save_body(c, PR.ASCII, precision)
    assert pcd.encode(c, PR.ASCII, precision) == want
    x0 = want.split(b"\n")[0].split(b" ")[0]
    assert x0 == b"nan"                                                   # the first x is the positive quiet NaN


def test_ascii_encode_known_text(pcd):
    c = {"x": bits([0xFFC00000, 0x80000000, 1]), "y": F32([np.inf, -np.inf, 0.1]), "z": F32([1.0, 2.5, -3.75]),
         "rgb": np.array([0xFF112233, 255, 0], np.uint32)}
    assert pcd.encode(c, PR.ASCII, 3) == b"-nan inf 1.000 1122867\n-0.000 -inf 2.500 255\n0.000 0.100 -3.750 0\n"


def test_ascii_encode_into_a_small_buffer(pcd):
    import ctypes as C
    from fastdem_amd import capi
    lib = capi.load()
    c = edge_cloud(())
    want = PR.save_body(c, PR.ASCII, 8)
    buf = np.full(len(want), 0xAA, dtype=np.uint8)
    need = C.c_uint64(0)
    p = [c[k].ctypes.data_as(C.c_void_p) for k in "xyz"]
    rc = lib.fdm_pcd_encode(c["x"].size, *p, None, None, None, None, None, 0, 0, 8, 0, buf.ctypes.data_as(C.c_void_p),
                            len(want) - 1, C.byref(need))
    assert rc == capi.FDM_SKIP_BUFFER_TOO_SMALL and need.value == len(want) and (buf == 0xAA).all()


def ascii_file(fields, lines, n=None, newline="\n"):
    n = len(lines) if n is None else n
    return ("FIELDS " + " ".join(fields) + f"\nWIDTH {n}\nDATA ascii\n").encode() + "".join(l + newline for l in lines).encode()


def tokens(v):
    return "%.9g" % float(v)


def decode_both(pcd, data):
    """(engine's channels or None on an error, the restatement's or None)."""
    from fastdem_amd import EngineError
    try:
        h = pcd.parse_header(data)
        got = pcd.decode(h, data[h.data_offset:])
    except EngineError:
        got = None
    try:
        want = PR.load(data)[1]
    except PR.PcdError:
        want = None
    return got, want


def assert_same_cloud(got, want):
    assert (got is None) == (want is None)
    if want is None:
        return
    for k in ("x", "y", "z", "intensity", "rgb", "nx", "ny", "nz"):
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            assert got[k].tobytes() == want[k].tobytes(), k


DECODE_FILES = {
    "plain": ascii_file(["x", "y", "z"], ["1 2 3", "-4.5 1e-3 +7", "0.1 0.2 0.3"]),
    "all_channels": ascii_file(["x", "y", "z", "intensity", "rgb", "normal_x", "normal_y", "normal_z"],
                               ["1 2 3 0.5 16711935 0 0 1", "4 5 6 255 4294967295 0.6 -0.8 0", "7 8 9 1e3 0 1 0 0"]),
    "special_values": ascii_file(["x", "y", "z", "i"], ["nan -nan inf -inf", "-0 0 -0.0 1e-30", "3.4028235e38 16777217 0.1 -1e-37",
                                                        "INF NaN Infinity 1.5"]),
    "edge_values_round_trip": ascii_file(["x", "y", "z"], [" ".join(tokens(v) for v in row) for row in
                                                           np.stack([edge_values()[13:]] * 3, 1)]),
    "count_is_not_accounted_for": ascii_file(["x", "y", "z", "pad", "intensity"], ["1 2 3 9 8 7 6", "4 5 6 1.5 2.5 3.5 4.5"]).replace(
        b"WIDTH", b"COUNT 1 1 1 3 1\nWIDTH"),
    "crlf_tabs_extra_tokens": ascii_file(["x", "y", "z", "rgba"], ["1\t2  3 7 extra", " 4 5 6 8\t"], newline="\r\n"),
    "no_final_newline": ascii_file(["x", "y", "z"], ["1 2 3", "4 5 6"])[:-1],
    "width_times_height": ascii_file(["x", "y", "z"], ["1 2 3"] * 6).replace(b"WIDTH 6", b"WIDTH 2\nHEIGHT 3"),
    "lines_behind_the_cloud": ascii_file(["x", "y", "z"], ["1 2 3", "4 5 6", "junk"], n=2),
    "empty_cloud": ascii_file(["x", "y", "z"], [], n=0),
    "number_then_text": ascii_file(["x", "y", "z", "rgb"], ["1.5abc 2e 3.x 12.9"]),
    "nx_ny_without_nz": ascii_file(["x", "y", "z", "nx", "ny"], ["1 2 3 4 5"]),
    # errors
    "too_few_lines": ascii_file(["x", "y", "z"], ["1 2 3"], n=2),
    "too_few_tokens": ascii_file(["x", "y", "z", "intensity"], ["1 2 3 4", "1 2 3"]),
    "empty_line_is_a_record": ascii_file(["x", "y", "z"], ["1 2 3", "", "4 5 6"], n=3),
    "not_a_number": ascii_file(["x", "y", "z"], ["1 two 3"]),
    "colour_not_a_number": ascii_file(["x", "y", "z", "rgb"], ["1 2 3 red"]),
    "out_of_range": ascii_file(["x", "y", "z"], ["1 2 1e39"]),
    "missing_z": ascii_file(["x", "y", "w"], ["1 2 3"]),
    "binary_word_but_ascii_needed": ascii_file(["x", "y", "z"], ["1 2 3"]).replace(b"DATA ascii", b"DATA"),
}
ERRORS = ["too_few_lines", "too_few_tokens", "empty_line_is_a_record", "not_a_number", "colour_not_a_number", "out_of_range",
          "missing_z"]


@pytest.mark.parametrize("name", sorted(DECODE_FILES))
def test_ascii_decode(pcd, name):
    got, want = decode_both(pcd, DECODE_FILES[name])
    assert (want is None) == (name in ERRORS)
    assert_same_cloud(got, want)


def test_ascii_decode_known_values(pcd):
    _, c = decode_both(pcd, DECODE_FILES["count_is_not_accounted_for"])
    assert c["intensity"].tolist() == [8.0, 2.5]
    _, c = decode_both(pcd, DECODE_FILES["all_channels"])
    assert c["rgb"].tolist() == [0xFF00FF, 0xFFFFFF, 0] and c["nz"].tolist() == [1.0, 0.0, 0.0]
    _, c = decode_both(pcd, DECODE_FILES["special_values"])
    assert np.isnan(c["x"][0]) and np.signbit(c["y"][0]) and c["x"][1].view(np.uint32) == 0x80000000
    assert c["y"][2] == F32(16777216.0)


def test_ascii_files_round_trip(pcd, tmp_path):
    c = edge_cloud(("intensity", "rgb", "normals"))
    path = str(tmp_path / "a.pcd")
    pcd.save_pcd(path, c, fmt=PR.ASCII, precision=8)
    with open(path, "rb") as f:
        assert f.read() == PR.save(c, PR.ASCII, 8)
    ok = {"x": F32([1.5, -2.25]), "y": F32([0.125, 3.0]), "z": F32([7.0, -0.5]), "intensity": F32([0.5, 1.0])}
    pcd.save_pcd(path, ok, fmt=PR.ASCII)
    back = pcd.load_pcd(path)
    for k in ("x", "y", "z", "intensity"):
        assert back[k].tobytes() == ok[k].tobytes()
    assert back["rgb"] is None and back["nx"] is None
