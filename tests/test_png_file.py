"""The PNG files of Engine.save_png (standard-library zlib) and of the C++ mirror's header-only writer
(fastdem/io/png.hpp: stored deflate blocks, own Adler-32) — the container checked chunk by chunk — and
fastdem::io::savePng on a mirror ElevationMap against the engine's pixels for the same scans."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from mirror_script import CPP_DEFAULTS
from test_render_gpu import COLS, RES, ROWS, T, restate_image, small_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "fastdem_amd", "cpp", "build")
PROBE = os.path.join(BUILD, "fdm_png_writer_probe")
TEST_PNG = os.path.join(BUILD, "fdm_test_png")


def decode_png(path):
    """A strict reader for what both writers promise: 8-bit RGBA, non-interlaced, filter 0 on every scanline.
    Returns (rgba uint8[height, width, 4], [chunk types], the zlib stream)."""
    with open(path, "rb") as f:
        b = f.read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    at, chunks = 8, []
    while at < len(b):
        (n,) = struct.unpack(">I", b[at:at + 4])
        kind, data = b[at + 4:at + 8], b[at + 8:at + 8 + n]
        assert len(data) == n, "truncated chunk"
        (crc,) = struct.unpack(">I", b[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + data) & 0xFFFFFFFF, f"CRC of {kind}"
        chunks.append((kind, data))
        at += 12 + n
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and chunks[-1][1] == b"" and b"IDAT" in kinds
    assert len(chunks[0][1]) == 13
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 6, 0, 0, 0), "8-bit RGBA, deflate, adaptive filter method, no interlace"
    z = b"".join(d for k, d in chunks if k == b"IDAT")
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof and d.unused_data == b"", "one complete zlib stream (its Adler-32 checked by zlib)"
    assert len(raw) == h * (1 + 4 * w), (len(raw), h, w)
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 4 * w)
    assert not lines[:, 0].any(), "filter type 0 on every scanline"
    return lines[:, 1:].reshape(h, w, 4).copy(), kinds, z


def pattern(w, h):
    r, c, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(4), indexing="ij")
    return ((7 * r + 13 * c + 29 * k + r * c) & 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- CPU part ----
def test_python_writer_container(tmp_path):
    from fastdem_amd.engine import write_png
    for w, h in ((150, 130), (1, 1), (48, 64)):
        path = str(tmp_path / f"p{w}x{h}.png")
        write_png(path, pattern(w, h))
        rgba, kinds, _ = decode_png(path)
        assert kinds == [b"IHDR", b"IDAT", b"IEND"]
        assert np.array_equal(rgba, pattern(w, h))


def test_python_writer_uses_no_imaging_library():
    src = open(os.path.join(ROOT, "fastdem_amd", "engine.py")).read()
    for name in ("PIL", "imageio", "cv2", "matplotlib", "png"):
        assert f"import {name}" not in src and f"from {name}" not in src, name


def test_cpp_writer_container(tmp_path):
    """fastdem/io/png.hpp's writer on fixed patterns: more than one 65 535-byte stored block, exactly one full block,
    and a 1 x 1 image."""
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fastdem_amd", "cpp")])
    r = subprocess.run([PROBE, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "written 1 refused 1" in r.stdout, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["big.png", "edge.png", "one.png"]
    for name, w, h in (("big.png", 150, 130), ("edge.png", 4, 3855), ("one.png", 1, 1)):
        rgba, kinds, z = decode_png(str(tmp_path / name))
        assert kinds == [b"IHDR", b"IDAT", b"IEND"]
        assert np.array_equal(rgba, pattern(w, h)), name
        # the stream is STORED blocks: 2 header bytes, 5 per block of at most 65 535 bytes, the Adler-32
        raw_len = h * (1 + 4 * w)
        blocks = max(1, -(-raw_len // 65535))
        assert len(z) == 2 + 5 * blocks + raw_len + 4, name
        assert z[:2] == b"\x78\x01" and struct.unpack(">I", z[-4:])[0] == zlib.adler32(
            np.concatenate([np.zeros((h, 1), np.uint8), pattern(w, h).reshape(h, 4 * w)], axis=1).tobytes())
        at = 2
        for k in range(blocks):  # every block header: BFINAL on the last only, LEN and its complement
            n = min(65535, raw_len - 65535 * k)
            assert z[at] == (1 if k == blocks - 1 else 0)
            assert struct.unpack("<HH", z[at + 1:at + 5]) == (n, n ^ 0xFFFF)
            at += 5 + n


# ---------------------------------------------------------------------------------------------------- GPU part ----
N_SCANS = 6
MOVE_TO = (0.93, -0.58)


def poses():
    return [T(0.21 * k, -0.13 * k) for k in range(N_SCANS)]


@pytest.mark.gpu
def test_engine_save_png(gpu, tmp_path):
    cfg = gpu.capi.default_config()
    eng = gpu.Engine(ROWS * RES, COLS * RES, RES, cfg)
    for k in range(3):
        s = small_scan(40 + k)
        eng.integrate(s["x"], s["y"], s["z"], T(z=0.6), poses()[k])
    for kw in ({}, {"normalize": "min_max", "colormap": "jet", "align_to_world": False}):
        path = str(tmp_path / "e.png")
        eng.save_png(path, "elevation", **kw)
        rgba, _, _ = decode_png(path)
        assert np.array_equal(rgba, eng.render_layer("elevation", **kw)[0])
        g = eng.geometry()
        assert np.array_equal(rgba, restate_image(eng.layer("elevation"), (g.start_row, g.start_col), **kw)[0])
    eng.close()


@pytest.mark.gpu
def test_cpp_save_png_against_the_engine(gpu, tmp_path):
    """fastdem::io::savePng on a mirror ElevationMap after six LOCAL-mode scans and a move: the decoded files hold the
    pixels Engine.render_layer gives for the same scans; a missing layer returns false and leaves no file."""
    assert os.path.exists(TEST_PNG), "build() makes fastdem_amd/cpp/build/fdm_test_png"
    scans = [small_scan(60 + k) for k in range(N_SCANS)]
    Tbs = T(z=0.6)
    with open(tmp_path / "scans.bin", "wb") as f:
        f.write(struct.pack("<I", N_SCANS))
        f.write(np.asarray(Tbs, dtype=np.float64).tobytes())
        for s, P in zip(scans, poses()):
            f.write(struct.pack("<I", s["x"].size))
            for c in ("x", "y", "z"):
                f.write(np.ascontiguousarray(s[c], dtype=np.float32).tobytes())
            f.write(np.asarray(P, dtype=np.float64).tobytes())
        f.write(struct.pack("<dd", *MOVE_TO))
    r = subprocess.run([TEST_PNG, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "png: ok" in r.stdout, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "missing.png")

    cfg = gpu.capi.default_config()
    for k, v in dict(CPP_DEFAULTS, mode=0).items():
        if k == "p2_dn":
            for i in range(5):
                cfg.p2_dn[i] = v[i]
        else:
            setattr(cfg, k, v)
    eng = gpu.Engine(ROWS * RES, COLS * RES, RES, cfg)
    for s, P in zip(scans, poses()):
        rc, _ = eng.integrate(s["x"], s["y"], s["z"], Tbs, P)
        assert rc == 0
    eng.move(*MOVE_TO)
    g = eng.geometry()
    assert g.start_row != 0 and g.start_col != 0
    assert f"start {g.start_row} {g.start_col}" in r.stdout
    for name, layer, kw in (("default.png", "elevation", {}),
                            ("minmax_jet.png", "variance", dict(normalize="min_max", colormap="jet", align_to_world=False)),
                            ("fixed_gray.png", "elevation", dict(normalize="fixed_range", colormap="grayscale",
                                                                 fixed=(np.float32(-0.2), np.float32(0.25))))):
        rgba, kinds, _ = decode_png(str(tmp_path / name))
        exp, _ = eng.render_layer(layer, **kw)
        assert rgba.shape == (ROWS, COLS, 4) and kinds == [b"IHDR", b"IDAT", b"IEND"]
        assert np.array_equal(rgba, exp), name
        assert np.array_equal(rgba, restate_image(eng.layer(layer), (g.start_row, g.start_col), **kw)[0]), name
        assert rgba[..., 3].any() and not rgba[..., 3].all(), name
    eng.close()
