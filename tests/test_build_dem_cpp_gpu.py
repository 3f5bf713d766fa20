"""fastdem/io/build_dem.hpp of the C++17 host mirror (fastdem_amd/cpp): the reference's BuildDEMTest gtests and nanoPCL's
statisticalOutlierRemoval tests re-expressed in fastdem_amd/cpp/tests/test_build_dem.cpp and run as a binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fastdem_amd", "cpp", "build", "fdm_test_build_dem")


def test_build_dem_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fastdem_amd", "cpp")])
    assert os.access(BIN, os.X_OK)


def test_the_pipeline_lives_in_a_header_of_its_own():
    inc = os.path.join(ROOT, "fastdem_amd", "cpp", "include", "fastdem", "io")
    code = "\n".join(line.split("//")[0] for line in open(os.path.join(inc, "build_dem.hpp")).read().splitlines())
    for name in ("struct DEMConfig", "buildDEM", "statisticalOutlierRemoval", "fdm_engine_build_dem"):
        assert name in code


@pytest.mark.gpu
def test_build_dem_spec_tests_on_gpu():
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and "10 tests" in r.stdout
