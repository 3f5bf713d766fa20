"""nanopcl/segmentation.hpp of the C++17 host mirror (fastdem_amd/cpp): nanoPCL's segmentation tests — its RANSAC group,
its ground group and the RANSAC / ground parts of its boundary group — re-expressed in
fastdem_amd/cpp/tests/test_segmentation.cpp, and the mirror's own (an index list, the refusals, the result's helpers), run
as a binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "fastdem_amd", "cpp")
BIN = os.path.join(CPP, "build", "fdm_test_segmentation")
NAMES = ("Ransac.plane_detection", "Ransac.plane_model_accuracy", "Ransac.inlier_outlier_split", "Ransac.multiple_planes",
         "Ransac.collinear_points", "Ransac.plane_from_points", "Ground.basic_segmentation", "Ground.grid_resolution",
         "Ground.thickness_config", "Ground.height_config", "Boundary.empty_cloud_ransac", "Boundary.empty_cloud_ground",
         "Boundary.single_point", "Boundary.insufficient_points_for_plane", "Mirror.index_list_and_errors")


def test_segmentation_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_segmentation_spec_tests_on_gpu(tmp_path):
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and f"{len(NAMES)} tests" in r.stdout
    for name in NAMES:
        assert f"[  OK  ] {name}" in r.stdout
