"""tests/filter_restate.py on the CPU: the two restatements of radius outlier removal — the reference's table and chains,
and the relation alone — give equal counts on every case of tests/filter_cases.py; every case is ADMITTED (finite, voxels
in range, on the lattice or one of tests/cluster_cases.py's admitted clouds, candidate tests under the work bound); the
cases hold what they were built for; the large case's constructor is the brute force at a few thousand points; the crop
restatements hold the NaN behaviour the reference's comparisons give.  Plus what runs without a device: the host algebra
(fastdem_amd/csrc/fdm_filter_host.hpp) stand-alone under the sanitizers, and the refusals that precede the device pick."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cluster_cases_large as CL
import cluster_restate as CR
import filter_cases as FC
import filter_restate as FR

F = np.float32
NAMES = sorted(FC.cases())
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_TESTS = 150_000_000_000  # filter::kMaxTests (fdm_filter_host.hpp)


# ------------------------------------------------------------------ radius outlier removal ----
@pytest.mark.parametrize("name", NAMES)
def test_the_two_restatements_agree(name):
    assert np.array_equal(FC.counts(name), FC.brute(name))


@pytest.mark.parametrize("name", NAMES)
def test_case_is_admitted(name):
    cloud, radius, _ = FC.cases()[name]
    pts = FC._pts(cloud)
    assert FR.admitted(pts, radius)
    assert CR.relation_constants(radius)[2] == 1
    assert FR.candidate_tests(pts, radius) <= MAX_TESTS
    if name not in FC.LATTICE_FREE:
        assert CL.on_the_lattice(cloud)
    else:  # (the lines and the spheres: tests/test_cluster_restate.py::test_case_is_admitted, at the same radius)
        assert CR.admission(*cloud, radius)[1] == 0


def test_the_cases_hold_what_they_were_built_for():
    c = FC.counts
    assert c("n0").size == 0 and c("n1").tolist() == [0] and c("n2_duplicate").tolist() == [1, 1] and c("n2_far").tolist() == [0, 0]
    assert (c("blob40_min1") == 39).all()
    assert {FC.cases()[f"blob40_min{s}"][2] for s in ("0", "1", "_n_1", "_n")} == {0, 1, 39, 40}
    assert c("exact_radius").tolist() == [6] + [1] * 6 + [0] * 5                 # `<=` at exactly the radius, none one step on
    assert sorted(c("faces_dyadic")[:27].tolist()) == [3] * 8 + [4] * 12 + [5] * 6 + [6] and not c("faces_dyadic")[27:].any()
    x, y, z = FC.cases()["signed_zeros"][0]
    assert np.signbit(x[:4]).any() and not np.signbit(x[:4]).all() and (c("signed_zeros")[:4] >= 3).all()
    for n in (255, 256, 257, 4097):                                              # the two ends of a line have one neighbour
        assert np.bincount(c(f"line{n}"), minlength=3).tolist() == [0, 2, n - 2]
    for name in ("negative_r03", "negative_r01"):
        assert all((v < 0).all() for v in FC.cases()[name][0][:2])
    # the dense voxel: ONE voxel of 5 000 and two outliers in neighbouring voxels, one of them in the own (y, z) row
    cloud, radius, min_neighbors = FC.cases()["dense_voxel"]
    pts = FC._pts(cloud)
    vox = CR.voxels(pts, CR.relation_constants(radius)[0])
    uniq, occupancy = np.unique(vox, axis=0, return_counts=True)
    assert sorted(map(tuple, uniq.tolist())) == [(0, 0, 0), (0, 1, 0), (1, 0, 0)] and sorted(occupancy.tolist()) == [1, 1, 5000]
    assert np.bincount(c("dense_voxel"), minlength=5000).tolist() == [2] + [0] * 4998 + [5000]
    assert FR.candidate_tests(pts, radius) == 5002 * 5001  # (the outliers' voxels are neighbours of each other too)
    # wide keys: more than 32 bits, and two occupied voxels share their low 32 bits
    cloud, radius, _ = FC.cases()["wide_33_bits"]
    bits, keys = __import__("cluster_cases").sort_keys(cloud, radius)
    assert bits == FC.KEY_BITS["wide_33_bits"] > 32 and np.unique(keys & 0xFFFFFFFF).size < np.unique(keys).size
    # every case's mask is no constant unless it was built to be one
    for name in NAMES:
        keep = c(name) >= FC.cases()[name][2]
        if name.startswith(("line", "negative", "spheres", "wide", "dense", "mixed", "exact", "faces")):
            assert keep.any() and not keep.all(), name


def test_no_fp32_radius_has_range_two():
    """The search the case module states: every radius of the binade [1, 2), none with radius * (1.0f / radius) > 1."""
    assert FC.range_two_radius() is None
    for r in (0.1, 0.3, 0.5, 1.0, 1e-3, 100.0, float(np.nextafter(F(1.0), F(2.0)))):
        assert CR.relation_constants(r)[2] == 1


def test_large_constructor_is_the_restatements_at_a_few_thousand_points():
    cloud, want = FC.blob_cloud(**FC.LARGE_SMALL)
    assert 4000 <= want.size <= 10000 and CL.on_the_lattice(cloud)
    pts = FC._pts(cloud)
    assert np.array_equal(FR.radius_counts_brute(pts, FC.RADIUS), want)
    assert np.array_equal(FR.radius_counts_reference(pts, FC.RADIUS), want)
    assert {0, 1, 2, 10} <= set(want.tolist())


def test_large_case_crosses_the_sorts_tile_switch():
    cloud, want = FC.large()
    n = want.size
    assert n == cloud[0].size > CL.RS_SMALL_MAX and n < CL.RS_SMALL_MAX + 20000  # just past it
    assert CL.on_the_lattice(cloud) and FR.admitted(FC._pts(cloud), FC.RADIUS)
    assert np.bincount(want)[:2].tolist() == [FC.LARGE["n_single"], 2 * FC.LARGE["n_pairs"] + 2 * 8000]
    keep = want >= 5
    assert keep.any() and not keep.all()
    assert FR.candidate_tests(FC._pts(cloud), FC.RADIUS) < 100_000_000


# ------------------------------------------------------------------ the crop restatements ----
def test_crop_restatements_hold_the_references_nan_behaviour():
    nan = np.nan
    x, y, z = (np.asarray(v, dtype=F) for v in ([nan, nan, 0.5, nan], [5.0, 0.5, nan, 0.5], [0.5, 0.5, 0.5, nan]))
    lo, hi = (-1.0, -2.0, 0.0), (2.0, 1.0, 1.5)
    assert FR.crop_box(x, y, z, lo, hi, "inside").tolist() == [False] * 4
    assert FR.crop_box(x, y, z, lo, hi, "outside").tolist() == [True, False, False, False]  # a NaN x, y outside: kept
    for mode in ("inside", "outside"):  # an axis crop drops a NaN coordinate in both modes
        assert not FR.crop_axis(x, -1.0, 2.0, mode)[[0, 1, 3]].any()
        assert not FR.crop_range(x, y, z, 1.0, 5.0, mode)[0]
    # cropAngle OUTSIDE keeps what INSIDE's expression calls false: a NaN is "not in range"
    assert not FR.crop_angle(x, y, z, -0.5, 0.5, "inside")[0] and FR.crop_angle(x, y, z, -0.5, 0.5, "outside")[0]
    assert FR.remove_invalid(x, y, z).tolist() == [False] * 4


def test_crop_cases_cover_both_outcomes_and_the_bounds():
    x, y, z = FC.crop_cloud()
    assert x.size == 1000 and np.isnan(x).any() and np.isinf(y).any() and np.signbit(x[x == 0]).any()
    for name, (fn, args, want) in FC.crop_cases().items():
        for mode, keep in want.items():
            assert keep.dtype == bool and keep.size == 1000
            if "min_above_max" in name:
                assert not keep.any() if mode == "inside" else keep.any()
            else:
                assert keep.any() and not keep.all(), (name, mode)
        if name != "finite":  # no mode is the other's negation: the NaN points are in neither, or in one by a comparison
            both = want["inside"] & want["outside"]
            assert not both.any()
            assert not (want["inside"] | want["outside"]).all() or name.startswith("angle")
    # the bounds themselves are inside (`>=`, `<=`), one ulp beyond is outside
    at = lambda px, py, pz: int(np.nonzero((x == F(px)) & (y == F(py)) & (z == F(pz)))[0][0])  # noqa: E731
    box = FC.crop_cases()["box"][2]
    assert box["inside"][at(-1.0, -2.0, 0.0)] and box["inside"][at(2.0, 1.0, 1.5)]
    assert box["outside"][at(np.nextafter(F(2.0), F(3.0)), 0.0, 0.5)]
    rng = FC.crop_cases()["range"][2]
    assert rng["inside"][at(3.0, 4.0, 0.0)] and rng["inside"][at(1.0, 0.0, 0.0)]            # exactly on both spheres
    assert rng["outside"][at(np.nextafter(F(5.0), F(6.0)), 0.0, 0.0)] and rng["outside"][at(np.nextafter(F(1.0), F(0.0)), 0.0, 0.0)]
    quarter = FC.crop_cases()["angle_quarter"][2]
    assert quarter["inside"][at(1.0, 1.0, 0.0)] and quarter["inside"][at(1.0, -1.0, 0.0)] and quarter["inside"][at(0.0, 0.0, 0.0)]
    # use_and: a span below pi is an intersection of half planes, so what lies behind the sensor is outside
    assert quarter["outside"][at(-1.0, 1.0, 0.0)] and quarter["outside"][at(-4.0, 0.0, 0.0)]
    assert FC.crop_cases()["angle_wrapped"][2]["inside"][at(-4.0, 0.0, 0.0)]
    assert FC.crop_cases()["angle_wide"][2]["inside"][at(4.0, 0.0, 0.0)] and FC.crop_cases()["angle_wide"][2]["outside"][at(-4.0, 0.0, 0.0)]


def test_angle_constants_are_libms():
    cos_min, sin_min, cos_max, sin_max, wrap, span, use_and = FR.angle_constants(3.0, -3.0)
    assert wrap and use_and and span == F(2.0) * F(np.pi) - F(6.0)
    assert abs(float(cos_min) - np.cos(3.0)) < 1e-7 and abs(float(sin_max) - np.sin(-3.0)) < 1e-7
    assert FR.angle_constants(0.0, FC.PI)[4:] == (False, F(np.pi), False)       # exactly pi: `<` fails
    assert FR.angle_constants(0.0, float(np.nextafter(F(np.pi), F(0.0))))[6]
    assert FR.angle_constants(1.0, 1.0)[4:] == (False, F(0.0), True)


# ------------------------------------------------------------------ the host algebra, stand-alone and sanitized ----
PROBE = os.path.join(ROOT, "fastdem_amd", "cpp", "tests", "filter_host_probe.cpp")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("filter_host") / "filter_host_probe")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "fastdem_amd", "csrc"), PROBE, "-o", exe])

    def run(numbers, expect=0):
        text = " ".join(float(v).hex() for v in numbers)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == expect, r.stdout[-2000:] + r.stderr[-4000:]
        return [float.fromhex(tok) for tok in r.stdout.split()]
    return run


def test_host_angle_algebra_holds_its_table(probe):
    assert probe((0,)) == [10.0]  # wrap, the span, use_and at exactly pi and an ulp below, min == max: the probe's table


def test_host_angle_constants_are_the_restatements(probe):
    rng = np.random.default_rng(5)
    pairs = [(-FC.PI / 4, FC.PI / 4), (3.0, -3.0), (0.0, FC.PI), (1.0, 1.0), (-2.0, 2.0), (1.0, -1.0), (FC.PI, -FC.PI)]
    pairs += [tuple(v) for v in rng.uniform(-7.0, 7.0, (40, 2)).astype(F).tolist()]
    for a, b in pairs:
        cos_min, sin_min, cos_max, sin_max, wrap, span, use_and = FR.angle_constants(a, b)
        assert probe((1, F(a), F(b))) == [float(cos_min), float(sin_min), float(cos_max), float(sin_max), float(span),
                                          float(wrap), float(use_and)], (a, b)


def test_host_keep_params(probe):
    lo, hi = (-1.0, -2.0, 0.25), (2.0, 1.0, 1.5)
    assert probe((2, 0, 1, *lo, *hi)) == [1.0, 0.0, 1.0, 0.0, *lo, *hi]
    assert probe((2, 1, 0, F(0.3), 9, 9, F(5.1), 9, 9)) == [1.0, 1.0, 0.0, 0.0, float(F(0.3) * F(0.3)), float(F(5.1) * F(5.1)), 0, 0, 0, 0]
    for kind in (2, 3, 4):
        assert probe((2, kind, 0, -1.0, 9, 9, 2.0, 9, 9)) == [1.0, float(kind), 0.0, 0.0, -1.0, 2.0, 0, 0, 0, 0]
    cs = FR.angle_constants(3.0, -3.0)
    assert probe((2, 5, 1, 3.0, 0, 0, -3.0, 0, 0)) == [1.0, 5.0, 1.0, 1.0, *map(float, cs[:4]), 0, 0]
    assert probe((2, 5, 0, 0.0, 0, 0, FC.PI, 0, 0))[3] == 0.0                   # exactly pi: OR
    assert probe((2, 6, 0, 1, 2, 3, 4, 5, 6)) == [1.0, 6.0, 0.0, 0.0] + [0.0] * 6
    for kind, mode in ((7, 0), (-1, 0), (0, 2), (0, -1)):
        assert probe((2, kind, mode, 0, 0, 0, 0, 0, 0)) == [0.0]


# ------------------------------------------------------------------ the refusals that need no device ----
def test_radius_and_null_arguments_are_refused_before_the_device_pick():
    import fastdem_amd as fdm
    x = np.zeros(8, dtype=F)
    for radius in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(fdm.EngineError, match="error -1: radius"):  # FDM_ERR_INVALID
            fdm.radius_outlier_removal(x, x, x, radius, 2)
    lib = fdm.capi.load()
    p = x.ctypes.data_as(C.c_void_p)
    keep = np.full(8, 0xAB, dtype=np.uint8)
    k = keep.ctypes.data_as(C.c_void_p)
    n_kept = C.c_uint64(7)
    for args in ((None, p, p, k), (p, None, p, k), (p, p, None, k), (p, p, p, None)):
        assert lib.fdm_cloud_radius_outlier_removal(8, *args[:3], 0, 0.5, 2, 0, args[3], None, C.byref(n_kept)) == -1
        assert b"null" in lib.fdm_last_error() and n_kept.value == 0
    assert lib.fdm_cloud_radius_outlier_removal(8, p, p, p, 0, 0.5, 2, 0, k, None, None) == -1
    assert lib.fdm_cloud_radius_outlier_removal(1 << 32, p, p, p, 0, 0.5, 2, 0, k, None, C.byref(n_kept)) == -1
    assert lib.fdm_cloud_radius_outlier_removal((1 << 32) - 4097, p, p, p, 0, 0.5, 2, 0, k, None, C.byref(n_kept)) == -1
    assert b"2^32-4097" in lib.fdm_last_error()
    assert (keep == 0xAB).all()
    # the crop entry: a kind or mode that does not exist, a null argument
    cfg = fdm.capi.FdmCropConfig(7, 0)
    assert lib.fdm_cloud_crop(8, p, p, p, 0, C.byref(cfg), 0, k, C.byref(n_kept)) == -1 and b"kind" in lib.fdm_last_error()
    cfg = fdm.capi.FdmCropConfig(0, 2)
    assert lib.fdm_cloud_crop(8, p, p, p, 0, C.byref(cfg), 0, k, C.byref(n_kept)) == -1 and b"mode" in lib.fdm_last_error()
    cfg = fdm.capi.FdmCropConfig(0, 0)
    assert lib.fdm_cloud_crop(8, p, p, p, 0, None, 0, k, C.byref(n_kept)) == -1
    assert lib.fdm_cloud_crop(8, None, p, p, 0, C.byref(cfg), 0, k, C.byref(n_kept)) == -1 and b"null" in lib.fdm_last_error()
    assert (keep == 0xAB).all()
    assert set(fdm.ror_last_stats()) == {"n_points", "candidate_tests", "tests_done", "n_kept", "range", "key_bits", "ms"}
