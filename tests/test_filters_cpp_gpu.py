"""nanopcl/filters/{core,crop,outlier_removal}.hpp in the C++17 host mirror (fastdem_amd/cpp): the filter cases of
nanoPCL's tests — removeInvalid, the crop group, the four radiusOutlierRemoval tests and the radius parts of its two
boundary tests — re-expressed in fastdem_amd/cpp/tests/test_filters.cpp through the mirror, and the mirror's own (the
const& and && overloads agree, channels and metadata are kept, the refusals), run as a binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "fastdem_amd", "cpp")
BIN = os.path.join(CPP, "build", "fdm_test_filters")
NAMES = ("Filters.removeInvalid", "Filters.cropBox_inside", "Filters.cropBox_outside", "Filters.cropRange", "Filters.cropZ",
         "Filters.radiusOutlierRemoval_basic", "Filters.radiusOutlierRemoval_all_inliers",
         "Filters.radiusOutlierRemoval_channel_preservation", "Filters.radiusOutlierRemoval_move",
         "Filters.outlierRemoval_empty_cloud", "Filters.outlierRemoval_single_point",
         "Mirror.overloads_agree", "Mirror.channels_and_metadata_kept", "Mirror.refusals")


def test_filter_tests_are_built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.access(BIN, os.X_OK)


@pytest.mark.gpu
def test_filter_spec_tests_on_gpu(tmp_path):
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and f"{len(NAMES)} tests" in r.stdout
    for name in NAMES:
        assert f"[  OK  ] {name}" in r.stdout
