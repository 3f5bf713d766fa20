"""The NumPy restatement of voxelized GICP (tests/vgicp_restate.py) against the reference's own known answers — the
VGICP cases of lib/nanoPCL/tests/test_registration.cpp, groups D and E, at the reference's tolerances and with its cloud
constructions under NumPy's generator — the admission of the align cases the device is held to (tests/vgicp_cases.py),
component checks of the map, and the mirror's host lookup built stand-alone under sanitizers.  No GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import reg_cases as RC
import reg_restate as RR
import vgicp_cases as VC
import vgicp_restate as VG
import voxel_restate as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def cloud_of(points):
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    return tuple(np.ascontiguousarray(p[:, a]) for a in range(3))


# ---- (a), (b): the reference's known answers; admission and spread ----
@pytest.mark.parametrize("name", VC.ALIGN_CASES)
def test_align_cases_meet_the_reference_and_are_admissible(name):
    case = VC.align_case(name)
    runs = [case.restated(order) for order in ("forward", "reversed", "pairwise")]
    a = runs[0]
    spread = max(float(np.linalg.norm(r.transform - a.transform)) for r in runs[1:])
    err = RR.transform_error(a.transform, case.gt)
    t_err, r_err = VC.pose_errors(a.transform, case.gt)
    print(f"{name}: {case.map.num_voxels} voxels, iterations {a.iterations}, converged {a.converged}, inliers "
          f"{a.num_inliers}/{case.problem.n}, fitness {a.fitness:.4f}, rmse {a.rmse:.3e}, error to truth {err:.3e} "
          f"(t {t_err:.4f} m, r {r_err:.4f} deg), spread {spread:.3e} (recorded {case.spread:.1e})")
    for r in runs[1:]:                                               # admitted: the three orders agree on every decision
        assert (r.iterations, r.converged, r.num_inliers) == (a.iterations, a.converged, a.num_inliers)
    assert spread <= 4.0 * case.spread            # (the record is the measurement; the factor is this check's own allowance)
    if name == "identity":                                           # test_vgicp_identity
        assert a.converged or err < 0.01
        assert err < case.tol
    if name == "convergence":                                        # test_vgicp_convergence
        assert a.converged and a.fitness > 0.1 and err < case.tol
    if case.limits is not None:                                      # test_vgicp_sparse_data
        assert t_err <= case.limits[0] and r_err <= case.limits[1]
    if name.startswith("designed"):
        VC.assert_gaps(case.map)
        assert a.converged and a.fitness == 1.0


def test_voxel_counts_and_iterations_of_the_reference_cases():
    """Pinned as measured when the cases were set up: a change of the restatement or of a cloud shows here first."""
    want = {"identity": (1370, 3), "convergence": (1370, 43), "very_sparse": (467, 8), "sparse": (927, 9),
            "moderate": (1887, 28), "dense": (4348, 49)}
    for name, (voxels, iterations) in want.items():
        case = VC.align_case(name)
        a = case.restated("forward")
        assert (case.map.num_voxels, a.iterations, a.converged) == (voxels, iterations, True), name


def test_the_huber_kernel_bites_on_the_designed_case():
    plain, huber = VC.align_case("designed_small"), VC.align_case("designed_huber")
    T = np.eye(4)
    assert huber.problem.linearize(T)["sums"][27] < VG.Problem(huber.source, huber.source_cov, huber.map).linearize(T)["sums"][27]
    assert plain.problem.set["robust_kernel"] == RR.NONE


def test_empty_source_and_empty_map_return_early():
    e = tuple(np.zeros(0, dtype=F32) for _ in range(3))
    c = VC.designed(300, (1, 2, 3, 4, 5, 8))
    cov = np.tile(np.eye(3, dtype=F32), (c[0].size, 1, 1))
    guess = RC.translation(1.0, 2.0, 3.0)
    for s, scov, m in ((e, cov[:0], VG.Map(*c, VC.EDGE)), (c, cov, VG.Map(*e, VC.EDGE)),
                       (c, cov, VG.Map(*(np.full(5, np.nan, dtype=F32),) * 3, VC.EDGE))):
        r = RR.align(VG.Problem(s, scov, m), guess)
        assert not r.converged and r.iterations == 0 and r.fitness == 0.0 and math.isinf(r.rmse)
        assert r.covariance is None and np.array_equal(r.transform, guess)


# ---- (c): components of the map ----
def test_designed_cloud_meets_its_condition():
    for nv, counts in ((500, (1, 2, 3, 4, 5, 8, 200)), (300, (1, 2, 3, 4, 5, 8))):
        m = VC.designed_map(nv, counts)
        print(f"designed {nv}: {m.n_points} points, {int(m.full.sum())} full voxels, smallest gap {m.min_gap():.3f}")
        VC.assert_gaps(m)
        assert m.num_voxels == nv and set(np.unique(m.count)) == set(counts)
        assert (VR.unpack(m.key)[0] < 0).any() and (VR.unpack(m.key)[2] < 0).any()
    random = VG.Map(*RC.sphere(5000, 42, 5.0), 0.5)                     # why the cloud is designed: a random one's gaps
    assert random.min_gap() < 1e-3


def test_counts_one_two_three_and_the_minus_zero_voxel():
    p = np.array([[-0.0, 0.1, 0.1], [-0.0, 0.2, 0.3], [-0.0, 0.4, 0.2]], dtype=F32)
    eps = 1e-3
    for n in (1, 2, 3):
        m = VG.Map(*cloud_of(p[:n]), 0.5, eps)
        assert m.num_voxels == 1 and m.count[0] == n
        assert np.signbit(m.sums[0, 0]) and np.signbit(m.mean[0, 0])    # assigned, then -0.0 + -0.0: never +0.0
        want = p[:n].astype(np.float64).sum(axis=0) / n
        assert np.allclose(m.mean[0, 1:], want[1:], rtol=1e-7)
        if n < 3:
            assert np.array_equal(m.cov[0], np.eye(3, dtype=F32) * F32(eps)) and np.array_equal(m.creg[0], np.eye(3))
        else:
            q = p.astype(np.float64)
            ref = (q[:, :, None] * q[:, None, :]).mean(axis=0) - np.outer(q.mean(axis=0), q.mean(axis=0))
            assert np.allclose(m.cov[0], ref, atol=1e-8) and m.cov[0, 0, 0] == 0.0
            w = np.linalg.eigvalsh(m.creg[0])
            assert np.allclose(w, [eps, 1.0, 1.0], atol=1e-12)          # V diag(eps, 1, 1) VT
            assert abs(abs(m.creg[0, 0, 0]) - eps) < 1e-12             # the flat direction is x
    both = VG.Map(*cloud_of([[0.0, 0.1, 0.1], [-0.0, 0.2, 0.3]]), 0.5)  # +0.0 first: the sum is +0.0
    assert not np.signbit(both.mean[0, 0])


def test_a_point_on_a_voxel_face_belongs_to_the_upper_voxel():
    m = VG.Map(*cloud_of([[0.5, 0.25, 0.25], [0.49999997, 0.25, 0.25], [-0.5, 0.25, 0.25], [-0.50000006, 0.25, 0.25]]), 0.5)
    assert VR.unpack(m.key)[0].tolist() == [-2, -1, 0, 1] and m.count.tolist() == [1, 1, 1, 1]
    assert m.rank_of(np.array([[0.5, 0.3, 0.3], [0.999, 0.0, 0.0], [1.0, 0.3, 0.3], [-0.5, 0.1, 0.1]])).tolist() == [3, 3, -1, 1]


def test_keys_are_clamped_at_plus_and_minus_two_to_the_twenty():
    m = VG.Map(*cloud_of([[2000.0, 0.0, 0.0], [1500.0, 0.0001, 0.0], [-2000.0, 0.0, 0.0], [-1048.576, 0.0, 0.0],
                          [1e30, -1e30, 1e30]]), 0.001)
    ix, iy, iz = VR.unpack(m.key)
    assert ix.tolist() == [-(1 << 20), -(1 << 20), (1 << 20) - 1] and m.count.tolist() == [1, 2, 2]
    assert (iy[0], iz[0]) == (-(1 << 20), -(1 << 20))                 # outside the int range: INT_MIN, clamped, for both signs
    assert (m.key >> np.uint64(63)).max() == 0                        # bit 63 is never set: ~0 can mark an empty slot


def test_points_that_are_not_finite_are_skipped():
    c = np.stack(VC.designed(300, (1, 2, 3, 4, 5, 8)), axis=1)
    bad = c[:30].copy()
    bad[np.arange(30), np.arange(30) % 3] = np.array([np.nan, np.inf, -np.inf], dtype=F32)[np.arange(30) // 3 % 3]
    mixed = np.insert(c, np.arange(0, 300, 10), bad, axis=0)
    a, b = VG.Map(*cloud_of(c), VC.EDGE), VG.Map(*cloud_of(mixed), VC.EDGE)
    assert b.n_skipped == 30 and np.array_equal(a.key, b.key) and a.mean.tobytes() == b.mean.tobytes()
    assert a.cov.tobytes() == b.cov.tobytes()


# ---- (d): the mirror's host lookup, stand-alone and sanitized ----
PROBE = os.path.join(ROOT, "fastdem_amd", "cpp", "tests", "vgicp_host_probe.cpp")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("vgicp_host") / "vgicp_host_probe")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "fastdem_amd", "cpp", "include"), PROBE, "-o", exe])

    def run(inv, keys, points):
        numbers = [float(inv), float(len(keys))]
        for k in keys:
            numbers += [float(int(k) >> 32), float(int(k) & 0xFFFFFFFF)]
        numbers += [float(len(points))] + [float(v) for v in np.asarray(points, dtype=F32).reshape(-1)]
        r = subprocess.run([exe], input=" ".join(v.hex() for v in numbers), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = np.array([float.fromhex(tok) for tok in r.stdout.split()]).reshape(-1, 3)
        return (out[:, 0].astype(np.uint64) << np.uint64(32)) | out[:, 1].astype(np.uint64), out[:, 2].astype(np.int64)
    return run


def check_probe(probe, vmap, points, label):
    points = np.asarray(points, dtype=F32).reshape(-1, 3)
    key, at = probe(vmap.inv, vmap.key, points)
    _, want_key = VR.keys_of(points[:, 0], points[:, 1], points[:, 2], vmap.resolution)
    finite = np.isfinite(points).all(axis=1)
    assert np.array_equal(key[finite], want_key[finite]), label
    want = vmap.rank_of(points)
    assert np.array_equal(np.where(at == vmap.num_voxels, -1, at)[finite], want[finite]), label
    return want


def test_host_lookup_packs_and_searches_as_the_restatement(probe):
    c = VC.designed(300, (1, 2, 3, 4, 5, 8))
    m = VG.Map(*c, VC.EDGE)
    g = np.random.default_rng(3)
    own = np.stack(c, axis=1)
    want = check_probe(probe, m, own, "the map's own points")
    assert (want >= 0).all()
    around = own[:400] + g.uniform(-0.6, 0.6, size=(400, 3)).astype(F32)
    want = check_probe(probe, m, around, "points around them")
    assert (want >= 0).any() and (want < 0).any()
    edges = [[0.5, 0.0, -0.5], [-0.0, 0.0, 0.0], [1e30, -1e30, 1e30], [-6.0, 5.999999, 6.0], [3e9, -3e9, 2147483648.0 * 0.5],
             [np.nan, 0.0, 0.0], [np.inf, -np.inf, 0.0]]                 # (the last two: no crash; their key is not compared)
    check_probe(probe, m, edges, "edges")
    check_probe(probe, VG.Map(*cloud_of([[2000.0, 0.0, 0.0], [-2000.0, 0.0, 0.0], [0.0, 0.0, 0.0]]), 0.001),
                [[2000.0, 0.0, 0.0], [1234.0, 0.0002, 0.0], [-5000.0, 0.0, 0.0], [0.0005, 0.0005, 0.0005], [1.0, 1.0, 1.0]], "clamped")
    # first and last key, one key, no key
    check_probe(probe, m, [own[np.argmin(m.rank_of(own))], own[np.argmax(m.rank_of(own))]], "first and last")
    check_probe(probe, VG.Map(*cloud_of([[0.1, 0.1, 0.1]]), VC.EDGE), [[0.2, 0.2, 0.2], [0.7, 0.2, 0.2], [-0.2, 0.2, 0.2]], "one key")
    check_probe(probe, VG.Map(*cloud_of(np.zeros((0, 3))), VC.EDGE), [[0.2, 0.2, 0.2]], "no key")
