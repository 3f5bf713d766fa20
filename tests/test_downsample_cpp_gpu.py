"""nanopcl/filters/downsample.hpp of the C++17 host mirror (fastdem_amd/cpp): nanoPCL's voxelGrid and gridMaxZ tests
re-expressed in fastdem_amd/cpp/tests/test_downsample.cpp, and the mirror's own (channel layout, refused sizes, the
process-wide order), run as a binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "fastdem_amd", "cpp")
BIN = os.path.join(CPP, "build", "fdm_test_downsample")
NAMES = ("VoxelGrid.centroid", "VoxelGrid.nearest", "VoxelGrid.channel_averaging", "VoxelGrid.move_semantics",
         "VoxelGrid.covariance_preservation", "VoxelGrid.symmetry", "GridMaxZ.basic", "GridMaxZ.multiple_cells",
         "GridMaxZ.channel_preservation", "EdgeCases.empty_cloud", "EdgeCases.single_point",
         "EdgeCases.nan_handling_in_voxelGrid", "Mirror.layout_metadata_and_every_mode",
         "Mirror.sizes_outside_the_range_throw", "Mirror.the_order_setting_decides_ties")


def test_downsample_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_downsample_spec_tests_on_gpu(tmp_path):
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and f"{len(NAMES)} tests" in r.stdout
    for name in NAMES:
        assert f"[  OK  ] {name}" in r.stdout
