"""fastdem/io/pcd_convert.hpp of the C++17 host mirror (fastdem_amd/cpp): the reference's rasterization gtests
re-expressed in fastdem_amd/cpp/tests/test_pcd_convert.cpp and run as a binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fastdem_amd", "cpp", "build", "fdm_test_pcd_convert")


def test_pcd_convert_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fastdem_amd", "cpp")])
    assert os.access(BIN, os.X_OK)


def test_the_mirror_does_not_declare_the_offline_dem_pipeline():
    """buildDEM (outlier removal, histogram filter) is out of scope: a missing symbol, not one that throws."""
    inc = os.path.join(ROOT, "fastdem_amd", "cpp", "include", "fastdem")
    src = open(os.path.join(inc, "io", "pcd_convert.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "buildDEM" not in code and "DEMConfig" not in code
    for name in ("fromPointCloud", "toPointCloud", "RasterMethod"):
        assert name in code
    assert "enum class RasterMethod" in open(os.path.join(inc, "config", "rasterization.hpp")).read()


@pytest.mark.gpu
def test_pcd_convert_spec_tests_on_gpu():
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and "18 tests" in r.stdout
