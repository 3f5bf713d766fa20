"""nanopcl/registration.hpp of the C++17 host mirror (fastdem_amd/cpp): nanoPCL's registration tests, its convergence
group B and stability group C, re-expressed in fastdem_amd/cpp/tests/test_registration.cpp, and the mirror's own (the
reference's exceptions for a missing channel, the result's helpers, the deleted alignVGICP overloads), run as a binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "fastdem_amd", "cpp")
BIN = os.path.join(CPP, "build", "fdm_test_registration")
NAMES = ("Convergence.icp_identity", "Convergence.icp_simple_translation", "Convergence.icp_rotation_translation",
         "Convergence.plane_icp", "Convergence.gicp", "Convergence.gicp_identity", "Stability.empty_cloud",
         "Stability.sparse_cloud", "Stability.bad_initial_guess", "Stability.partial_overlap",
         "Mirror.missing_channels_throw_as_in_the_reference", "Mirror.result_helpers", "Mirror.vgicp_overloads_are_deleted")


def test_registration_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_registration_spec_tests_on_gpu(tmp_path):
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and f"{len(NAMES)} tests" in r.stdout
    for name in NAMES:
        assert f"[  OK  ] {name}" in r.stdout
