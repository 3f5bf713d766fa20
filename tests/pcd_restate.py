"""Plain Python / NumPy restatement of nanoPCL's PCD reader and writer, written from the reference's source and not from
the engine — the reading the engine is held to (tests/test_pcd_*.py).  Test data, not product.

  parse_header   detail::parseHeader, fastdem/lib/nanoPCL/include/nanopcl/io/pcd_io.hpp:114-207, plus the field choice
                 of loadPCD :260-281
  load           loadPCD :243-378 with readFieldAsFloat :209-230
  save           savePCD :415-550

What std::stoul / std::stod / std::stof do with a token is restated for decimal text only (an optional sign, digits, a
fraction, an exponent, inf, nan); hexadecimal floats are not.  A token they reject raises PcdError, as does every place
where the reference indexes a missing token.

Run as a program it rewrites the fixtures under tests/golden/pcd/.
"""
import math
import os
import re
import struct
from fractions import Fraction

import numpy as np

F32 = np.float32
ASCII, BINARY = 0, 1
MAX_FIELDS = 64      # the engine's fixed-layout header holds no more (the reference has no bound)
MAX_POINT_SIZE = 1024


class PcdError(Exception):
    pass


SPACE = " \t\n\v\f\r"          # what `iss >> token` skips in the "C" locale


def split(line):               # detail::split (:104-112)
    return [t for t in re.split("[ \t\n\v\f\r]+", line) if t]


def lower(s):                  # std::tolower per char, "C" locale: ASCII letters only
    return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in s)


def stoul_u32(tok):
    """static_cast<uint32_t>(std::stoul(tok)) on a 64-bit unsigned long."""
    m = re.match(r"[+-]?[0-9]+", tok)
    if not m:
        raise PcdError(f"stoul: {tok!r}")
    v = int(m.group(0).lstrip("+-"))
    if v > 2 ** 64 - 1:
        raise PcdError(f"stoul out of range: {tok!r}")
    if m.group(0).startswith("-"):
        v = (2 ** 64 - v) % 2 ** 64
    return v & 0xFFFFFFFF


_FLOAT = re.compile(r"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?|[nN][aA][nN])")


def _prefix(tok, what):
    m = _FLOAT.match(tok)
    if not m:
        raise PcdError(f"{what}: {tok!r}")
    return m.group(0)


def stod(tok):
    s = _prefix(tok, "stod")
    v = float(s)
    if math.isinf(v) and "inf" not in s.lower():
        raise PcdError(f"stod out of range: {tok!r}")
    return v


def stof(tok):
    """std::stof: the decimal text rounded ONCE to the nearest float (ties to even); out of range raises."""
    s = _prefix(tok, "stof")
    low = s.lower().lstrip("+-")
    neg = s.startswith("-")
    if low.startswith("inf"):
        return F32(-np.inf if neg else np.inf)
    if low.startswith("nan"):
        return F32(np.nan) if not neg else -F32(np.nan)
    exact = Fraction(s)
    with np.errstate(over="ignore"):
        near = F32(float(s))                       # rounded twice: at most one float off
    if not np.isfinite(near):
        near = F32(np.finfo(F32).max) * (-1 if neg else 1)
    with np.errstate(over="ignore"):
        cands = {float(near), float(np.nextafter(near, F32(np.inf))), float(np.nextafter(near, F32(-np.inf)))}
    best = None
    for c in cands:
        if not math.isfinite(c):
            continue
        d = abs(Fraction(c) - exact)
        even = (int(F32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, c)
    v = F32(best[1])
    top = Fraction(float(np.finfo(F32).max))
    if abs(exact) >= top + Fraction(2) ** 103:       # half an ulp above FLT_MAX rounds to infinity: ERANGE
        raise PcdError(f"stof out of range: {tok!r}")
    if exact != 0 and abs(exact) < Fraction(float(np.finfo(F32).tiny)) and Fraction(float(v)) != exact:
        raise PcdError(f"stof underflow: {tok!r}")   # glibc: a tiny, inexact result sets ERANGE, and stof throws
    if v == 0 and neg:
        v = F32(-0.0)
    return v


class Field:
    def __init__(self, name, type_, size, count, offset):
        self.name, self.type, self.size, self.count, self.offset = name, type_, size, count, offset

    def __repr__(self):
        return f"Field({self.name!r}, {self.type!r}, {self.size}, {self.count}, {self.offset})"


class Header:
    def __init__(self):
        self.fields = []
        self.width, self.height, self.point_size = 0, 1, 0
        self.viewpoint = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)     # tx ty tz qw qx qy qz
        self.format = ASCII
        self.data_offset = 0
        self.idx = {}

    @property
    def num_points(self):
        return (self.width * self.height) & 0xFFFFFFFF              # :88, uint32

    def find(self, name):                                           # :90-95
        for i, f in enumerate(self.fields):
            if f.name == name:
                return i
        return -1


def parse_header(data):
    """parseHeader over bytes; Header.data_offset is where the stream stands afterwards."""
    h = Header()
    names, sizes, types, counts = [], [], [], []
    pos, n = 0, len(data)
    while pos < n:                                                  # std::getline (:123)
        nl = data.find(b"\n", pos)
        end = n if nl < 0 else nl
        line = data[pos:end].decode("latin-1")
        pos = n if nl < 0 else nl + 1
        if line == "" or line[0] == "#":
            continue
        tok = split(line)
        if not tok:
            continue
        key = lower(tok[0])
        if key == "fields":
            names += [lower(t) for t in tok[1:]]
        elif key == "size":
            sizes += [stoul_u32(t) for t in tok[1:]]
        elif key == "type":
            types += [t[0] for t in tok[1:]]
        elif key == "count":
            counts += [stoul_u32(t) for t in tok[1:]]
        elif key in ("width", "height"):
            if len(tok) < 2:
                raise PcdError(f"{key} without a number")           # tokens[1] of a one-token line (:150, :152)
            setattr(h, key, stoul_u32(tok[1]))
        elif key == "viewpoint":
            if len(tok) >= 8:
                h.viewpoint = tuple(stod(t) for t in tok[1:8])
        elif key == "data":
            if len(tok) >= 2:
                fmt = lower(tok[1])
                if fmt == "ascii":
                    h.format = ASCII
                elif fmt == "binary":
                    h.format = BINARY
                elif fmt == "binary_compressed":
                    raise PcdError("binary_compressed")
            break
    h.data_offset = pos
    if not names:
        raise PcdError("missing FIELDS")
    if len(names) > MAX_FIELDS:
        raise PcdError("more than 64 fields")
    offset = 0
    for i, name in enumerate(names):
        size = sizes[i] if i < len(sizes) else 4
        type_ = types[i] if i < len(types) else "F"
        count = counts[i] if i < len(counts) else 1                 # (an empty COUNT list: all 1, :189-191)
        h.fields.append(Field(name, type_, size, count, offset))
        offset = (offset + size * count) & 0xFFFFFFFF
    h.point_size = offset

    def first(*alias):
        for a in alias:
            if h.find(a) >= 0:
                return h.find(a)
        return -1
    h.idx = {"x": h.find("x"), "y": h.find("y"), "z": h.find("z"), "intensity": first("intensity", "i", "reflectivity"),
             "rgb": first("rgb", "rgba"), "nx": first("normal_x", "nx"), "ny": first("normal_y", "ny"),
             "nz": first("normal_z", "nz")}
    return h


def read_field_as_float(rec, field):                                # :209-230
    o = field.offset
    if field.type == "F" and field.size == 4:
        return np.frombuffer(rec, dtype="<f4", count=1, offset=o)[0]          # bits copied
    if field.type == "F" and field.size == 8:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return np.frombuffer(rec, dtype="<f8", count=1, offset=o).astype(F32)[0]
    if field.type == "U" and field.size == 1:
        return F32(rec[o])
    if field.type == "U" and field.size == 4:
        return F32(struct.unpack_from("<I", rec, o)[0])
    if field.type == "I" and field.size == 4:
        return F32(struct.unpack_from("<i", rec, o)[0])
    return F32(0.0)


def _read_width(field):
    pair = (field.type, field.size)
    return {("F", 4): 4, ("F", 8): 8, ("U", 1): 1, ("U", 4): 4, ("I", 4): 4}.get(pair, 0)


def load_body(h, body):
    """The data section of loadPCD: dict of x, y, z (float32), intensity, rgb (uint32 0x00RRGGBB), nx, ny, nz — the
    optional ones None when the file lacks the channel.  Raises PcdError where the reference throws, and for the layouts
    it leaves undefined (see the module's callers: the engine refuses them too)."""
    n = h.num_points
    ix = h.idx
    has_i, has_c = ix["intensity"] >= 0, ix["rgb"] >= 0
    has_n = ix["nx"] >= 0 and ix["ny"] >= 0 and ix["nz"] >= 0
    out = {"x": np.zeros(n, F32), "y": np.zeros(n, F32), "z": np.zeros(n, F32),
           "intensity": np.zeros(n, F32) if has_i else None, "rgb": np.zeros(n, np.uint32) if has_c else None,
           "nx": np.zeros(n, F32) if has_n else None, "ny": np.zeros(n, F32) if has_n else None,
           "nz": np.zeros(n, F32) if has_n else None}
    if n == 0:                                                      # :255
        return {k: (None if k not in "xyz" else v) for k, v in out.items()}
    if ix["x"] < 0 or ix["y"] < 0 or ix["z"] < 0:
        raise PcdError("missing x, y, z")
    floats = ["x", "y", "z"] + (["intensity"] if has_i else []) + (["nx", "ny", "nz"] if has_n else [])
    if h.format == ASCII:
        pos = 0
        for i in range(n):
            if pos >= len(body):
                raise PcdError("unexpected end of ASCII data")      # getline fails (:299)
            nl = body.find(b"\n", pos)
            end = len(body) if nl < 0 else nl
            tok = split(body[pos:end].decode("latin-1"))
            pos = len(body) if nl < 0 else nl + 1
            if len(tok) < len(h.fields):
                raise PcdError(f"incomplete point data at line {i}")
            for k in floats:
                out[k][i] = stof(tok[ix[k]])                        # the token at the field's INDEX (:308-328)
            if has_c:
                out["rgb"][i] = stoul_u32(tok[ix["rgb"]]) & 0xFFFFFF
        return out
    # binary (:332-375)
    ps = h.point_size
    if ps == 0:
        raise PcdError("point size 0 (undefined in the reference)")
    if ps > MAX_POINT_SIZE:
        raise PcdError("point size above 1024 (the engine's bound)")
    for k in floats:
        f = h.fields[ix[k]]
        if f.offset + _read_width(f) > ps:
            raise PcdError("field reaches beyond the record (undefined in the reference)")
    if has_c and h.fields[ix["rgb"]].offset + 4 > ps:
        raise PcdError("colour field reaches beyond the record (undefined in the reference)")
    if len(body) < n * ps:
        raise PcdError("unexpected end of binary data")
    for i in range(n):
        rec = bytes(body[i * ps:(i + 1) * ps])
        for k in floats:
            out[k][i] = read_field_as_float(rec, h.fields[ix[k]])
        if has_c:
            out["rgb"][i] = struct.unpack_from("<I", rec, h.fields[ix["rgb"]].offset)[0] & 0xFFFFFF
    return out


def load(data):
    h = parse_header(data)
    return h, load_body(h, data[h.data_offset:])


def fmt_g(v):
    """operator<<(double) at a stream's defaults: %g, six significant digits."""
    return "%g" % v


def fmt_fixed(v, precision):
    """operator<<(float) under std::fixed: "%.*f" of the value widened to double."""
    v = F32(v)
    if np.isnan(v):
        return "-nan" if np.signbit(v) else "nan"
    return "%.*f" % (precision, float(v))


def save_header(n, has_intensity, has_rgb, has_normal, viewpoint=None, fmt=BINARY):          # :427-491, :516
    names, sizes, types = ["x", "y", "z"], ["4"] * 3, ["F"] * 3
    if has_intensity:
        names, sizes, types = names + ["intensity"], sizes + ["4"], types + ["F"]
    if has_rgb:
        names, sizes, types = names + ["rgb"], sizes + ["4"], types + ["U"]
    if has_normal:
        names, sizes, types = names + ["normal_x", "normal_y", "normal_z"], sizes + ["4"] * 3, types + ["F"] * 3
    vp = viewpoint if viewpoint is not None else (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
    text = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\n"
    text += "FIELDS " + " ".join(names) + "\nSIZE " + " ".join(sizes) + "\nTYPE " + " ".join(types) + "\n"
    text += "COUNT" + " 1" * len(names) + "\n"
    text += f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT " + " ".join(fmt_g(v) for v in vp) + f"\nPOINTS {n}\n"
    text += "DATA ascii\n" if fmt == ASCII else "DATA binary\n"
    return text.encode("ascii")


def save_body(c, fmt=BINARY, precision=8):
    """The data section of savePCD for a dict as load_body returns it (absent channels None or missing)."""
    n = len(c["x"])
    has_i, has_c = c.get("intensity") is not None, c.get("rgb") is not None
    has_n = all(c.get(k) is not None for k in ("nx", "ny", "nz"))
    if fmt == BINARY:
        cols = [np.asarray(c[k], F32).view(np.uint32) for k in "xyz"]
        if has_i:
            cols.append(np.asarray(c["intensity"], F32).view(np.uint32))
        if has_c:
            cols.append(np.asarray(c["rgb"], np.uint32) & np.uint32(0xFFFFFF))
        if has_n:
            cols += [np.asarray(c[k], F32).view(np.uint32) for k in ("nx", "ny", "nz")]
        return np.stack(cols, 1).astype("<u4").tobytes() if n else b""
    lines = []
    for i in range(n):
        t = [fmt_fixed(c[k][i], precision) for k in "xyz"]
        if has_i:
            t.append(fmt_fixed(c["intensity"][i], precision))
        if has_c:
            t.append(str(int(c["rgb"][i]) & 0xFFFFFF))
        if has_n:
            t += [fmt_fixed(c[k][i], precision) for k in ("nx", "ny", "nz")]
        lines.append(" ".join(t) + "\n")
    return "".join(lines).encode("ascii")


def save(c, fmt=BINARY, precision=8, viewpoint=None):
    has_n = all(c.get(k) is not None for k in ("nx", "ny", "nz"))
    return save_header(len(c["x"]), c.get("intensity") is not None, c.get("rgb") is not None, has_n, viewpoint, fmt) + \
        save_body(c, fmt, precision)


# ------------------------------------------------------------------------------------------------- fixtures ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcd")


def three_points():
    """The hand-built cloud of tests/test_pcd_restate.py."""
    return {"x": np.array([1.0, -2.5, 0.0], F32), "y": np.array([0.5, 1e-3, -0.0], F32),
            "z": np.array([3.0, 100.25, 1e10], F32), "intensity": np.array([0.0, 0.5, 255.0], F32),
            "rgb": np.array([0x112233, 0xFF0000, 0x0000FF], np.uint32), "nx": None, "ny": None, "nz": None}


def slope_cloud(n=300, seed=5):
    """A small noisy slope with intensity and colour: the file the pcd2dem tool is run on."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n)
    z = 0.2 * x + rng.normal(0.0, 0.01, n)
    return {"x": x.astype(F32), "y": y.astype(F32), "z": z.astype(F32), "intensity": rng.uniform(0, 1, n).astype(F32),
            "rgb": rng.integers(0, 1 << 24, n).astype(np.uint32), "nx": None, "ny": None, "nz": None}


def fixtures():
    return {"three_points_binary.pcd": save(three_points(), BINARY), "three_points_ascii.pcd": save(three_points(), ASCII),
            "slope_binary.pcd": save(slope_cloud(), BINARY)}


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    for name, data in fixtures().items():
        with open(os.path.join(GOLDEN, name), "wb") as f:
            f.write(data)
        print(name, len(data))
