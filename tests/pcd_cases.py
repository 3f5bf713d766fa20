"""Header texts and record layouts shared by the PCD tests (tests/test_pcd_*.py).  Test data, not product."""
import struct

import numpy as np

import pcd_restate as PR

F32 = np.float32

VALID = (b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity rgb\nSIZE 4 4 4 4 4\n"
         b"TYPE F F F F U\nCOUNT 1 1 1 1 1\nWIDTH 12\nHEIGHT 3\nVIEWPOINT 1 2 3 0.5 0.5 -0.5 0.5\nPOINTS 36\nDATA binary\n")


def many_fields(k):
    return ("FIELDS " + " ".join(["x", "y", "z"] + [f"f{i}" for i in range(k - 3)]) + "\nWIDTH 1\nDATA ascii\n").encode()


# name -> header bytes; what each must give is what tests/pcd_restate.py gives (an error included)
HEADERS = {
    "valid": VALID,
    "crlf": VALID.replace(b"\n", b"\r\n"),
    "comments_and_blanks": b"# one\n\nVERSION 0.7\n# two\n\n\nFIELDS x y z\n   \n#three\nWIDTH 2\n\t\nDATA ascii\n1 2 3\n",
    "upper_case": b"VERSION .7\nFIELDS X Y Z Intensity RGB\nSIZE 4 4 4 4 4\nTYPE F F F F U\nWIDTH 5\nHEIGHT 1\nDATA BINARY\n",
    "lower_case_keys_and_types": b"fields x y z\nsize 4 4 4\ntype f f f\ncount 1 1 1\nwidth 4\ndata Binary\n",
    "short_lists": b"FIELDS x y z intensity\nSIZE 8 8\nTYPE F\nCOUNT 1 1 2\nWIDTH 3\nDATA binary\n",
    "no_lists": b"FIELDS x y z\nWIDTH 3\nDATA ascii\n",
    "count4_padding": (b"FIELDS x y z _ intensity _\nSIZE 4 4 4 1 4 1\nTYPE F F F U F U\n"
                       b"COUNT 1 1 1 4 1 4\nWIDTH 7\nDATA binary\n"),
    "pcl_xyzrgbnormal": (b"FIELDS x y z _ normal_x normal_y normal_z _ rgb curvature _\nSIZE 4 4 4 1 4 4 4 1 4 4 1\n"
                         b"TYPE F F F U F F F U U F U\nCOUNT 1 1 1 4 1 1 1 4 1 1 8\nWIDTH 257\nDATA binary\n"),
    "missing_data": b"FIELDS x y z\nWIDTH 2\nHEIGHT 2\n",
    "data_without_word": b"FIELDS x y z\nWIDTH 2\nDATA\n1 2 3\n",
    "data_unknown_word": b"FIELDS x y z\nWIDTH 2\nDATA zipped\n1 2 3\n",
    "data_without_newline": b"FIELDS x y z\nWIDTH 0\nDATA binary",
    "binary_compressed": b"FIELDS x y z\nWIDTH 2\nDATA binary_compressed\n",
    "no_fields": b"VERSION 0.7\nSIZE 4 4 4\nWIDTH 2\nDATA ascii\n",
    "empty": b"",
    "width_without_number": b"FIELDS x y z\nWIDTH\nDATA ascii\n",
    "height_without_number": b"FIELDS x y z\nWIDTH 1\nHEIGHT \nDATA ascii\n",
    "width_not_a_number": b"FIELDS x y z\nWIDTH many\nDATA ascii\n",
    "width_number_then_text": b"FIELDS x y z\nWIDTH 12abc\nDATA ascii\n",
    "size_not_a_number": b"FIELDS x y z\nSIZE 4 four 4\nWIDTH 1\nDATA ascii\n",
    "negative_width": b"FIELDS x y z\nWIDTH -1\nHEIGHT 1\nDATA ascii\n",
    "width_times_height_wraps": b"FIELDS x y z\nWIDTH 65536\nHEIGHT 65537\nDATA ascii\n",
    "points_ignored": b"FIELDS x y z\nWIDTH 3\nHEIGHT 2\nPOINTS 99\nDATA ascii\n",
    "height_default": b"FIELDS x y z\nWIDTH 9\nDATA ascii\n",
    "viewpoint_six_numbers": b"FIELDS x y z\nWIDTH 1\nVIEWPOINT 1 2 3 1 0 0\nDATA ascii\n",
    "viewpoint_eight_numbers": b"FIELDS x y z\nWIDTH 1\nVIEWPOINT 1.5 -2 3e2 0 1 0 0 77\nDATA ascii\n",
    "viewpoint_not_a_number": b"FIELDS x y z\nWIDTH 1\nVIEWPOINT 1 2 3 a 0 0 0\nDATA ascii\n",
    "fields_64": many_fields(64),
    "fields_65": many_fields(65),
    "fields_on_two_lines": b"FIELDS x y\nFIELDS z intensity\nSIZE 4 4 4 1\nTYPE F F F U\nWIDTH 1\nDATA binary\n",
    "alias_intensity_first": b"FIELDS reflectivity x i y intensity z\nWIDTH 1\nDATA ascii\n",
    "alias_i_before_reflectivity": b"FIELDS reflectivity x i y z\nWIDTH 1\nDATA ascii\n",
    "alias_reflectivity": b"FIELDS reflectivity x y z\nWIDTH 1\nDATA ascii\n",
    "alias_rgb_over_rgba": b"FIELDS rgba x y z rgb\nWIDTH 1\nDATA ascii\n",
    "alias_rgba": b"FIELDS x y z rgba\nWIDTH 1\nDATA ascii\n",
    "alias_normal_mixed": b"FIELDS x y z nx normal_y nz normal_x\nWIDTH 1\nDATA ascii\n",
    "nx_ny_without_nz": b"FIELDS x y z nx ny\nWIDTH 1\nDATA ascii\n",
    "duplicate_x": b"FIELDS x y z x\nWIDTH 1\nDATA ascii\n",
    "no_z": b"FIELDS x y\nWIDTH 1\nDATA ascii\n",
    "hash_inside_line": b" # FIELDS a\nFIELDS x y z # w\nWIDTH 1\nDATA ascii\n",
    "tabs_and_spaces": b"FIELDS\tx  y\t z\nSIZE\t4 4 4\nWIDTH\t\t3\nDATA\tascii\n",
}


def header_tuple(h):
    """A restated Header as plain values, comparable with engine_tuple."""
    ix = h.idx
    return ([(f.name, f.type, f.size, f.count, f.offset) for f in h.fields], h.width, h.height, h.point_size,
            tuple(h.viewpoint), h.format, h.data_offset,
            (ix["x"], ix["y"], ix["z"], ix["intensity"], ix["rgb"], ix["nx"], ix["ny"], ix["nz"]))


def engine_tuple(h):
    """An fdm_pcd_header as the same plain values."""
    return ([(f.name.decode("latin-1"), f.type.decode("latin-1"), f.size, f.count, f.offset) for f in h.fields[:h.n_fields]],
            h.width, h.height, h.point_size, tuple(h.viewpoint), h.format, h.data_offset,
            (h.idx_x, h.idx_y, h.idx_z, h.idx_intensity, h.idx_rgb, h.idx_nx, h.idx_ny, h.idx_nz))


def restated(data):
    """header_tuple of the restatement's parse, or None where it raises."""
    try:
        return header_tuple(PR.parse_header(data))
    except PR.PcdError:
        return None


def digest(t):
    """One line for a header tuple: what cpp/tests/pcd_host_probe.cpp prints for a parse."""
    if t is None:
        return "error"
    fields, width, height, point_size, vp, fmt, off, idx = t
    return (f"ok {len(fields)} {width} {height} {point_size} {fmt} {off} " + " ".join(str(i) for i in idx) + " " +
            " ".join(f"{n}:{ord(ty)}:{s}:{c}:{o}" for n, ty, s, c, o in fields) + " vp " + " ".join("%.17g" % v for v in vp))


# ---- binary record layouts: (fields line items) -> header + records ----
def layout_header(fields, n, fmt="binary"):
    """fields: list of (name, type, size, count)."""
    return ("FIELDS " + " ".join(f[0] for f in fields) + "\nSIZE " + " ".join(str(f[2]) for f in fields) + "\nTYPE " +
            " ".join(f[1] for f in fields) + "\nCOUNT " + " ".join(str(f[3]) for f in fields) +
            f"\nWIDTH {n}\nHEIGHT 1\nPOINTS {n}\nDATA {fmt}\n").encode()


def xyz_f4(extra=()):
    return [("x", "F", 4, 1), ("y", "F", 4, 1), ("z", "F", 4, 1)] + list(extra)


def pad(k):
    return ("_", "U", 1, k)


LAYOUTS = {   # point_size -> fields
    3: [("x", "U", 1, 1), ("y", "U", 1, 1), ("z", "U", 1, 1)],
    12: xyz_f4(),
    13: xyz_f4([("intensity", "U", 1, 1)]),
    16: xyz_f4([("intensity", "F", 4, 1)]),
    19: xyz_f4([("intensity", "F", 4, 1), ("ring", "U", 2, 1), ("flag", "U", 1, 1)]),
    32: xyz_f4([("intensity", "F", 4, 1), ("rgb", "U", 4, 1), ("normal_x", "F", 4, 1), ("normal_y", "F", 4, 1),
                ("normal_z", "F", 4, 1)]),
    48: [("x", "F", 4, 1), ("y", "F", 4, 1), ("z", "F", 4, 1), pad(4), ("normal_x", "F", 4, 1), ("normal_y", "F", 4, 1),
         ("normal_z", "F", 4, 1), pad(4), ("rgb", "U", 4, 1), ("curvature", "F", 4, 1), pad(8)],
    128: xyz_f4([pad(100), ("rgba", "U", 4, 1), ("i", "I", 4, 1), ("nx", "F", 8, 1)]),          # the LDS path's last size
    129: xyz_f4([pad(101), ("rgba", "U", 4, 1), ("i", "I", 4, 1), ("nx", "F", 8, 1)]),          # the direct path's first
    255: xyz_f4([pad(235), ("intensity", "F", 8, 1)]),
    256: xyz_f4([pad(236), ("intensity", "F", 8, 1)]),
    257: xyz_f4([pad(1), ("intensity", "U", 4, 1), pad(236), ("rgb", "F", 4, 1)]),
    1024: xyz_f4([("pad", "F", 4, 250), ("intensity", "I", 4, 1), ("rgb", "U", 4, 1), ("z2", "F", 4, 1)]),
    1025: xyz_f4([pad(1013)]),
}


def random_records(fields, n, seed):
    """n records of random bytes with plausible floats in x, y, z where those are F4: every byte of every field is
    arbitrary otherwise (NaN payloads, infinities and subnormals included)."""
    rng = np.random.default_rng(seed)
    size = sum(f[2] * f[3] for f in fields)
    rec = rng.integers(0, 256, (n, size), dtype=np.uint8)
    off = 0
    for name, type_, sz, count in fields:
        if name in ("x", "y", "z") and type_ == "F" and sz == 4:
            v = rng.uniform(-100, 100, n).astype("<f4")
            keep = rng.random(n) < 0.25               # a quarter of them stay random bit patterns
            col = rec[:, off:off + 4].copy()
            col[~keep] = v.view(np.uint8).reshape(n, 4)[~keep]
            rec[:, off:off + 4] = col
        off += sz * count
    return rec.tobytes()


def special_values():
    """(header, body): x F8, y F4, z F8, intensity U4, rgba with a top byte, nx I4, ny U1, nz F4 — the conversions'
    edge cases, one record each."""
    f8 = [0.0, -0.0, 1.0, float(np.finfo(F32).tiny) / 2, 1e-45, 7e-46, 2.0 ** -150, 3.5e38, -3.5e38, 3.4028235677973366e38,
          1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, float("inf"), float("-inf"), float("nan"),
          1e-320, 16777217.0, -1e300]
    f4_bits = [0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x7F7FFFFF, 0x7FA00000, 0, 0x80000000]
    u4 = [0, 1, 16777216, 16777217, 16777219, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 129, 2 ** 32 - 128]
    i4 = [0, -1, -2 ** 31, 2 ** 31 - 1, 16777217, -16777217]
    n = len(f8)
    fields = [("x", "F", 8, 1), ("y", "F", 4, 1), ("z", "F", 8, 1), ("intensity", "U", 4, 1), ("rgba", "U", 4, 1),
              ("nx", "I", 4, 1), ("ny", "U", 1, 1), ("nz", "F", 4, 1)]
    body = b""
    for i in range(n):
        body += struct.pack("<dIdIIiBI", f8[i], f4_bits[i % len(f4_bits)], f8[(i + 5) % n], u4[i % len(u4)],
                            0xAB000000 | (i * 0x010203), i4[i % len(i4)], (i * 37) % 256, f4_bits[(i + 3) % len(f4_bits)])
    return layout_header(fields, n), body


# (type, size) pairs readFieldAsFloat has no branch for: they read as 0
UNSUPPORTED = [("U", 2), ("I", 1), ("I", 2), ("I", 8), ("U", 8), ("F", 2), ("f", 4), ("u", 4), ("i", 4), ("u", 1), ("f", 8),
               ("D", 8), ("X", 4)]


def unsupported_layout(type_, size):
    """x and intensity of the given pair, y and z F4 after them."""
    return [("x", type_, size, 1), ("intensity", type_, size, 1), ("y", "F", 4, 1), ("z", "F", 4, 1)]
