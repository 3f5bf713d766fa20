"""nanopcl/geometry/normal_estimation.hpp of the C++17 host mirror (fastdem_amd/cpp): nanoPCL's seventeen normal /
covariance estimation tests re-expressed in fastdem_amd/cpp/tests/test_geometry.cpp, and the mirror's own (the refusal of
more than 64 neighbours, the deleted radius overloads), run as a binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "fastdem_amd", "cpp")
BIN = os.path.join(CPP, "build", "fdm_test_geometry")
NAMES = ("Normals.plane_xy", "Normals.plane_xz", "Normals.plane_arbitrary", "Normals.viewpoint_orientation",
         "Normals.viewpoint_below", "Normals.sparse_cloud", "Normals.with_external_kdtree", "Covariances.planar",
         "Covariances.gicp_regularization", "Covariances.invalid_returns_identity", "Covariances.with_external_kdtree",
         "Combined.single_pass", "Combined.with_external_kdtree", "EdgeCases.empty_cloud", "EdgeCases.single_point",
         "EdgeCases.collinear_points", "EdgeCases.normal_unit_length", "Mirror.more_than_64_neighbours_throw",
         "Mirror.radius_overloads_are_deleted")


def test_geometry_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_geometry_spec_tests_on_gpu(tmp_path):
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and f"{len(NAMES)} tests" in r.stdout
    for name in NAMES:
        assert f"[  OK  ] {name}" in r.stdout
