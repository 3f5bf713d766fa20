"""nanopcl/registration/vgicp.hpp of the C++17 host mirror (fastdem_amd/cpp): nanoPCL's voxelized-GICP tests, groups D
and E, re-expressed in fastdem_amd/cpp/tests/test_vgicp.cpp at the reference's tolerances, and the mirror's own (the
map's accessors and host lookups, a moved map, the early returns, the reference's exception text), run as a binary.  The
header is opt-in: nanopcl/registration.hpp alone still declares alignVGICP deleted (tests/test_register_cpp_gpu.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "fastdem_amd", "cpp")
BIN = os.path.join(CPP, "build", "fdm_test_vgicp")
NAMES = ("VGICP.identity", "VGICP.convergence", "VGICP.sparse_data", "Mirror.map_accessors_and_host_lookups",
         "Mirror.early_returns_and_the_missing_covariances")


def test_vgicp_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.access(BIN, os.X_OK)


def test_including_registration_first_stops_with_the_fix(tmp_path):
    """registration.hpp before vgicp.hpp: an #error that names the fix, not a redefinition of a deleted function."""
    src = tmp_path / "late.cpp"
    src.write_text('#include "nanopcl/core.hpp"\n#include "nanopcl/registration/vgicp.hpp"\nint main() { return 0; }\n')
    inc = ["-I", os.path.join(CPP, "include"), "-I", os.path.join(ROOT, "include")]
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", *inc, str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "include nanopcl/registration/vgicp.hpp first, or compile with -DNANOPCL_VGICP" in r.stderr
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-DNANOPCL_VGICP", *inc, str(src)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.gpu
def test_vgicp_spec_tests_on_gpu(tmp_path):
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and f"{len(NAMES)} tests" in r.stdout
    for name in NAMES:
        assert f"[  OK  ] {name}" in r.stdout
