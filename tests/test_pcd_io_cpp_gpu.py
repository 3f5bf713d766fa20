"""nanopcl/io/pcd_io.hpp of the C++17 host mirror (fastdem_amd/cpp) and the pcd2dem tool: nanoPCL's six PCD tests
re-expressed in fastdem_amd/cpp/tests/test_pcd_io.cpp plus a pcd2dem-shaped round trip, run as a binary; and
build/pcd2dem on a fixture, whose output file must equal, byte for byte, what fastdem_amd.pcd.pcd2dem writes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "fastdem_amd", "cpp")
BIN = os.path.join(CPP, "build", "fdm_test_pcd_io")
TOOL = os.path.join(CPP, "build", "pcd2dem")
FIXTURE = os.path.join(ROOT, "tests", "golden", "pcd", "slope_binary.pcd")


def test_pcd_io_tests_and_the_tool_are_built():
    if not (os.path.exists(BIN) and os.path.exists(TOOL)):
        subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.access(BIN, os.X_OK) and os.access(TOOL, os.X_OK)


def test_the_tool_prints_its_usage():
    r = subprocess.run([TOOL], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr.startswith("Usage: pcd2dem <input.pcd> <output.pcd> [resolution]\n")


@pytest.mark.gpu
def test_pcd_io_spec_tests_on_gpu(tmp_path):
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and "7 tests" in r.stdout
    for name in ("pcd_ascii_roundtrip", "pcd_binary_roundtrip", "pcd_viewpoint", "pcd_rgb_channel", "pcd_empty_cloud",
                 "pcd_exception_on_bad_stream", "pcd2dem_roundtrip"):
        assert f"[  OK  ] PcdIO.{name}" in r.stdout


@pytest.mark.gpu
def test_the_tool_writes_what_the_python_entry_point_writes(gpu, tmp_path):
    out_tool, out_py = str(tmp_path / "tool.pcd"), str(tmp_path / "py.pcd")
    r = subprocess.run([TOOL, FIXTURE, out_tool, "0.2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    n = gpu.pcd.pcd2dem(FIXTURE, out_py, gpu.DEMConfig(resolution=0.2))
    assert n > 50
    with open(out_tool, "rb") as a, open(out_py, "rb") as b:
        assert a.read() == b.read()
    lines = r.stdout.splitlines()
    assert lines[0] == f"Loading {FIXTURE} ..." and lines[1] == "  300 points"
    assert lines[2] == "Building DEM (resolution=0.2m) ..." and lines[3].startswith("  Grid: ") and lines[3].endswith(" cells")
    assert lines[4] == f"  {n} elevation cells" and lines[5] == f"Saved to {out_tool}"
    # a file whose cloud leaves no map: 0 points out of both, and a file that is no PCD: an error, no crash
    empty = str(tmp_path / "empty.pcd")
    with open(empty, "wb") as f:
        f.write(b"FIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nWIDTH 0\nDATA binary\n")
    r = subprocess.run([TOOL, empty, out_tool], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "  0 elevation cells" in r.stdout, r.stdout + r.stderr
    assert gpu.pcd.pcd2dem(empty, out_py) == 0
    with open(out_tool, "rb") as a, open(out_py, "rb") as b:
        assert a.read() == b.read()
    for bad in (str(tmp_path), str(tmp_path / "missing.pcd")):          # a directory, a missing file
        r = subprocess.run([TOOL, bad, out_tool], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and r.stderr.startswith("pcd2dem: "), (bad, r.returncode, r.stderr)
