"""Known answers of the PCD restatement itself (tests/pcd_restate.py): a hand-built file byte for byte, and one case per
rule of nanoPCL's parseHeader / loadPCD / savePCD (nanopcl/io/pcd_io.hpp:114-550) that is easy to get wrong."""
import os
import struct

import numpy as np
import pytest

import pcd_restate as PR

F32 = np.float32

HEAD = (b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity rgb\nSIZE 4 4 4 4 4\n"
        b"TYPE F F F F U\nCOUNT 1 1 1 1 1\nWIDTH 3\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 3\nDATA %s\n")
BINARY_BODY = (struct.pack("<ffffI", 1.0, 0.5, 3.0, 0.0, 0x112233) + struct.pack("<ffffI", -2.5, 1e-3, 100.25, 0.5, 0xFF0000) +
               struct.pack("<ffffI", 0.0, -0.0, 1e10, 255.0, 0x0000FF))
ASCII_BODY = (b"1.00000000 0.50000000 3.00000000 0.00000000 1122867\n"
              b"-2.50000000 0.00100000 100.25000000 0.50000000 16711680\n"
              b"0.00000000 -0.00000000 10000000000.00000000 255.00000000 255\n")


def test_hand_built_files_byte_for_byte():
    c = PR.three_points()
    assert PR.save(c, PR.BINARY) == HEAD % b"binary" + BINARY_BODY
    assert PR.save(c, PR.ASCII) == HEAD % b"ascii" + ASCII_BODY
    for data in (HEAD % b"binary" + BINARY_BODY, HEAD % b"ascii" + ASCII_BODY):
        h, got = PR.load(data)
        assert (h.width, h.height, h.num_points, h.point_size) == (3, 1, 3, 20)
        for k in ("x", "y", "z", "intensity", "rgb"):
            assert got[k].tobytes() == c[k].tobytes(), k
        assert got["nx"] is None


def test_fixtures_are_what_the_restatement_writes():
    for name, data in PR.fixtures().items():
        with open(os.path.join(PR.GOLDEN, name), "rb") as f:
            assert f.read() == data, name


def parse(text):
    return PR.parse_header(text.encode())


def test_comments_and_empty_lines_are_skipped():
    h = parse("# c\n\nFIELDS x y z\n#WIDTH 9\n\nWIDTH 2\nDATA ascii\n")
    assert h.width == 2 and [f.name for f in h.fields] == ["x", "y", "z"]


def test_a_trailing_cr_is_white_space():
    h = parse("FIELDS x y z\r\nWIDTH 2\r\nDATA binary\r\n")
    assert h.fields[2].name == "z" and h.width == 2 and h.format == PR.BINARY and h.data_offset == 36


def test_keys_and_names_are_lower_cased():
    h = parse("fIeLdS X Y Z RGB\nwidth 1\nDaTa BINARY\n")
    assert [f.name for f in h.fields] == ["x", "y", "z", "rgb"] and h.format == PR.BINARY and h.idx["rgb"] == 3


def test_type_keeps_its_case_and_a_lower_case_f_reads_as_zero():
    h = parse("FIELDS x y z\nSIZE 4 4 4\nTYPE f F Float\nWIDTH 1\nDATA binary\n")
    assert [f.type for f in h.fields] == ["f", "F", "F"]
    c = PR.load_body(h, struct.pack("<fff", 1.0, 2.0, 3.0))
    assert (c["x"][0], c["y"][0], c["z"][0]) == (0.0, 2.0, 3.0)


def test_defaults_of_short_lists():
    h = parse("FIELDS a b c d\nSIZE 8\nTYPE U U\nCOUNT 3 1 2\nWIDTH 1\nDATA ascii\n")
    assert [(f.size, f.type, f.count) for f in h.fields] == [(8, "U", 3), (4, "U", 1), (4, "F", 2), (4, "F", 1)]
    assert [f.offset for f in h.fields] == [0, 24, 28, 36] and h.point_size == 40


def test_num_points_is_width_times_height_in_uint32_and_points_is_ignored():
    assert parse("FIELDS x\nWIDTH 3\nHEIGHT 4\nPOINTS 5\nDATA ascii\n").num_points == 12
    assert parse("FIELDS x\nWIDTH 7\nDATA ascii\n").num_points == 7
    assert parse("FIELDS x\nWIDTH 65536\nHEIGHT 65537\nDATA ascii\n").num_points == 65536


def test_viewpoint_needs_seven_numbers():
    assert parse("FIELDS x\nVIEWPOINT 1 2 3 0 1 0\nDATA ascii\n").viewpoint == (0, 0, 0, 1, 0, 0, 0)
    assert parse("FIELDS x\nVIEWPOINT 1 2 3 0 1 0 0 9\nDATA ascii\n").viewpoint == (1, 2, 3, 0, 1, 0, 0)


def test_data_ends_the_header():
    text = "FIELDS x y z\nWIDTH 1\nDATA binary\nWIDTH 5\n"
    h = parse(text)
    assert h.width == 1 and h.data_offset == text.index("WIDTH 5")
    assert parse("FIELDS x\nDATA binary").data_offset == len("FIELDS x\nDATA binary")


@pytest.mark.parametrize("line,fmt", [("DATA ascii", PR.ASCII), ("DATA binary", PR.BINARY), ("DATA", PR.ASCII),
                                      ("DATA lzf", PR.ASCII), ("", PR.ASCII)])
def test_data_formats(line, fmt):
    assert parse(f"FIELDS x\nWIDTH 1\n{line}\n").format == fmt


@pytest.mark.parametrize("text", ["FIELDS x\nDATA binary_compressed\n", "WIDTH 1\nDATA ascii\n", "FIELDS x\nWIDTH\nDATA ascii\n",
                                  "FIELDS x\nHEIGHT\n", "FIELDS x\nWIDTH w\n", "FIELDS x\nSIZE 4x 4\nCOUNT z\n",
                                  "FIELDS x\nVIEWPOINT 0 0 0 1 0 0 q\n", "FIELDS x\nWIDTH 99999999999999999999\n"])
def test_header_errors(text):
    with pytest.raises(PR.PcdError):
        parse(text)


def test_field_choice():
    ix = parse("FIELDS reflectivity i x y z rgba rgb nx normal_y nz normal_x\nDATA ascii\n").idx
    assert (ix["intensity"], ix["rgb"], ix["nx"], ix["ny"], ix["nz"]) == (1, 6, 10, 8, 9)
    h = parse("FIELDS x y z nx ny\nWIDTH 1\nDATA ascii\n")
    assert PR.load_body(h, b"1 2 3 4 5\n")["nx"] is None          # the normal channel needs all three
    with pytest.raises(PR.PcdError):
        PR.load_body(parse("FIELDS x y\nWIDTH 1\nDATA ascii\n"), b"1 2\n")


def test_read_field_as_float_pairs():
    rec = struct.pack("<fdBIi", 1.5, 1.0 + 2.0 ** -24, 200, 2 ** 32 - 1, -2 ** 31)
    F = PR.Field
    assert PR.read_field_as_float(rec, F("a", "F", 4, 1, 0)) == F32(1.5)
    assert PR.read_field_as_float(rec, F("a", "F", 8, 1, 4)) == F32(1.0)            # half an ulp: to even
    assert PR.read_field_as_float(rec, F("a", "U", 1, 1, 12)) == F32(200.0)
    assert PR.read_field_as_float(rec, F("a", "U", 4, 1, 13)) == F32(4294967296.0)
    assert PR.read_field_as_float(rec, F("a", "I", 4, 1, 17)) == F32(-2147483648.0)
    for t, s in (("U", 2), ("I", 1), ("I", 2), ("I", 8), ("U", 8), ("F", 2), ("f", 4), ("X", 4)):
        assert PR.read_field_as_float(rec, F("a", t, s, 1, 0)) == 0.0
    nan = struct.pack("<I", 0x7FA12345)
    assert PR.read_field_as_float(nan, F("a", "F", 4, 1, 0)).view(np.uint32) == 0x7FA12345


def test_binary_records():
    h = parse("FIELDS x y z rgba\nSIZE 4 4 4 1\nTYPE F F F U\nCOUNT 1 1 1 4\nWIDTH 2\nDATA binary\n")
    body = struct.pack("<fffI", np.nan, np.inf, 1.0, 0xAB123456) + struct.pack("<fffI", 1, 2, 3, 7) + b"extra"
    c = PR.load_body(h, body)
    assert np.isnan(c["x"][0]) and np.isinf(c["y"][0]) and c["rgb"].tolist() == [0x123456, 7]      # nothing is dropped
    with pytest.raises(PR.PcdError):
        PR.load_body(h, body[:31])                                                  # a short body
    with pytest.raises(PR.PcdError):                                                # colour's 4 bytes leave the record
        PR.load_body(parse("FIELDS x y z rgb\nSIZE 4 4 4 1\nTYPE F F F U\nWIDTH 1\nDATA binary\n"), bytes(13))
    with pytest.raises(PR.PcdError):
        PR.load_body(parse("FIELDS x y z\nSIZE 0 0 0\nWIDTH 1\nDATA binary\n"), b"")   # point_size 0


def test_ascii_records():
    h = parse("FIELDS x y z pad intensity\nCOUNT 1 1 1 3 1\nWIDTH 2\nDATA ascii\n")
    c = PR.load_body(h, b"1 2 3 9 8 7 6\n4 5 6 1.5 2.5\r\n")
    assert c["intensity"].tolist() == [8.0, 2.5]        # the token at the field's index: COUNT is not accounted for
    with pytest.raises(PR.PcdError):
        PR.load_body(h, b"1 2 3 4 5\n")                 # getline fails
    with pytest.raises(PR.PcdError):
        PR.load_body(h, b"1 2 3 4 5\n1 2 3 4\n")        # fewer tokens than fields
    with pytest.raises(PR.PcdError):
        PR.load_body(h, b"1 2 3 4 5\n\n1 2 3 4 5\n")    # an empty line is a record
    assert PR.stof("0.1") == F32(0.1) and PR.stof("2.5e0x") == F32(2.5)
    assert PR.stof("16777217") == F32(16777216.0) and PR.stof("-0").view(np.uint32) == 0x80000000
    with pytest.raises(PR.PcdError):
        PR.stof("1e39")
    assert PR.stoul_u32("4294967297") == 1 and PR.stoul_u32("-1") == 0xFFFFFFFF and PR.stoul_u32("12.5") == 12


def test_save_header_and_ascii_format():
    vp = (1.5, -2.0, 1e-7, 0.70710678118654757, 0.0, 0.70710678118654746, 0.0)
    text = PR.save_header(5, False, True, True, vp, PR.ASCII).decode()
    assert "FIELDS x y z rgb normal_x normal_y normal_z\nSIZE 4 4 4 4 4 4 4\nTYPE F F F U F F F\nCOUNT 1 1 1 1 1 1 1\n" in text
    assert "WIDTH 5\nHEIGHT 1\nVIEWPOINT 1.5 -2 1e-07 0.707107 0 0.707107 0\nPOINTS 5\nDATA ascii\n" in text
    assert PR.fmt_fixed(F32(0.1), 8) == "0.10000000" and PR.fmt_fixed(F32(-0.0), 3) == "-0.000"
    assert PR.fmt_fixed(F32(np.inf), 8) == "inf" and PR.fmt_fixed(-F32(np.inf), 8) == "-inf"
    assert PR.fmt_fixed(np.uint32(0x7FC00000).view(F32), 8) == "nan" and PR.fmt_fixed(np.uint32(0xFFC00000).view(F32), 8) == "-nan"
    assert PR.fmt_fixed(np.uint32(1).view(F32), 8) == "0.00000000"
    assert PR.fmt_fixed(F32(3.4028235e38), 1) == "340282346638528859811704183484516925440.0"
