"""nanopcl/segmentation.hpp's euclideanCluster in the C++17 host mirror (fastdem_amd/cpp): the clustering cases of
nanoPCL's segmentation tests — its Euclidean group, the clustering parts of its boundary group, its channel test and its
two pipeline tests — re-expressed in fastdem_amd/cpp/tests/test_cluster.cpp through the mirror's four overloads, extract
and applyClusterLabels, and the mirror's own (the overloads agree, the stated order, the refusals), run as a binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "fastdem_amd", "cpp")
BIN = os.path.join(CPP, "build", "fdm_test_cluster")
NAMES = ("Euclidean.basic_clustering", "Euclidean.csr_format", "Euclidean.cluster_extraction", "Euclidean.config_tolerance",
         "Euclidean.config_min_max_size", "Euclidean.subset_clustering", "Euclidean.apply_labels", "Euclidean.noise_indices",
         "Boundary.empty_cloud_clustering", "Boundary.single_point_clustering",
         "Channels.cluster_extract_preserves_channels", "Integration.ground_removal_then_clustering",
         "Integration.ransac_then_clustering", "Mirror.overloads_agree_and_order_is_stated", "Mirror.refusals")


def test_cluster_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_cluster_spec_tests_on_gpu(tmp_path):
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and f"{len(NAMES)} tests" in r.stdout
    for name in NAMES:
        assert f"[  OK  ] {name}" in r.stdout
