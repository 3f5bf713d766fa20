"""tests/cluster_restate.py on the CPU: the restatement satisfies the assertions nanoPCL's own tests make about
euclideanCluster (tests/test_segmentation.cpp:111-277, :504-509, :523-531, :555-584), its partition equals the
brute-force connected components of the relation on every case of tests/cluster_cases.py, every cluster's first BFS
element is its smallest position (the seed), every case is ADMITTED, and the canonical form — what tests/test_cluster_gpu.py
compares the device with — is the stable-sort reading of the restatement's own order.

The large cases (tests/cluster_cases_large.py) take their answers from their construction; here the same constructors
are run at a few thousand points against the BFS and the brute force, the cases are shown to be on the lattice (their
admission) and to cross the thresholds they were built for, and each is shown to be SENSITIVE: the computation with the
targeted branch skipped gives another answer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cluster_cases as CC
import cluster_cases_large as CL
import cluster_restate as CR
import seg_cases_large as SL

F = np.float32
NAMES = sorted(CC.cases())
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(name):
    cloud, kw = CC.cases()[name]
    return cloud, kw.get("tolerance", 0.5), kw.get("min_size", 10), kw.get("max_size", 100000), kw.get("indices")


def sizes(off):
    return np.diff(off.astype(np.int64)).tolist()


# ------------------------------------------------------------------ the reference's own assertions ----
def test_basic_clustering_and_csr():  # :111-145
    ind, off, _ = CC.restated("spheres")
    assert off.size - 1 == 3 and ind.size == 100
    assert off[0] == 0 and sum(sizes(off)) == ind.size and sizes(off) == [50, 30, 20]


def test_min_and_max_size():  # :189-207
    assert sizes(CC.restated("spheres_min25")[1]) == [50, 30]
    assert sizes(CC.restated("spheres_max40")[1]) == [30, 20]  # the oversized one is dropped whole


def test_tolerance_case():  # :166-187
    assert sizes(CC.restated("two_groups")[1]) == [20, 20]


def test_subset_indices_reference_the_cloud():  # :209-234
    cloud, kw = CC.cases()["ground_subset"]
    ind, off, _ = CC.restated("ground_subset")
    assert off.size - 1 >= 1 and (ind < cloud[0].size).all()
    assert set(ind.tolist()) <= set(kw["indices"].tolist()) and (cloud[2][ind] > F(0.5)).all()


def test_labels_and_noise():  # :236-277
    cloud, _ = CC.cases()["spheres"]
    ind, off, _ = CC.restated("spheres")
    lab = CR.apply_cluster_labels(ind, off, cloud[0].size, 1)
    assert lab.size == cloud[0].size and int(((lab & 0xFFFF) > 0).sum()) == ind.size and ((lab >> 16) == 1).all()
    ind, off, _ = CC.restated("line_noise")
    assert CR.noise_indices(ind, 52).tolist() == [50, 51]


def test_label_instance_id_is_truncated_to_16_bits():
    off = np.arange(0, 65538, dtype=np.uint32)  # 65 537 clusters of one point
    lab = CR.apply_cluster_labels(np.arange(65537, dtype=np.uint32), off, 65537, 3)
    assert lab[65534] == (3 << 16) | 65535 and lab[65535] == (3 << 16) and lab[65536] == (3 << 16) | 1


def test_empty_and_single_point():  # :504-509, :523-531
    ind, off, _ = CC.restated("m0")
    assert off.tolist() == [0] and ind.size == 0
    assert CC.restated("m1_min2")[1].tolist() == [0]
    assert CC.restated("m1_min1")[0].tolist() == [0]


def test_extract_case_gives_two_clusters():  # :555-584
    pts = [(F(i) * F(0.1), 0, 0) for i in range(20)] + [(F(10.0) + F(i) * F(0.1), 0, 0) for i in range(20)]
    x, y, z = (np.asarray([p[k] for p in pts], dtype=F) for k in range(3))
    _, off, _ = CR.euclidean_cluster(x, y, z, tolerance=0.5, min_size=10)
    assert sizes(off) == [20, 20]


# ------------------------------------------------------------------ what the cases were built to hold ----
def test_the_cases_hold_what_they_were_built_for():
    assert sizes(CC.restated("pair_exact")[1]) == [2] and sizes(CC.restated("pair_ulp")[1]) == [1, 1]
    assert sizes(CC.restated("faces_dyadic")[1]) == [27] + [1] * 27
    for n in (63, 64, 65, 255, 256, 257, 4097):
        assert sizes(CC.restated(f"line{n}")[1]) == [n] and sizes(CC.restated(f"diagonal{n}")[1]) == [n]
    assert sizes(CC.restated("interleaved257")[1]) == [257, 257]
    assert sizes(CC.restated("dense_voxel")[1]) == [3000, 2000]
    assert sizes(CC.restated("singletons_min1")[1]) == [1] * 20000 and sizes(CC.restated("singletons_min2")[1]) == []
    assert sizes(CC.restated("ties64x12")[1]) == [12] * 64
    assert CC.list_length("mixed70k") == 70000 and len(sizes(CC.restated("mixed70k")[1])) > 100
    # the dense voxel is ONE voxel; the range is 1 for every tolerance of the table
    cloud, tol, _, _, _ = config("dense_voxel")
    pts, _ = CR._points(*cloud, None)
    assert np.unique(CR.voxels(pts, CR.relation_constants(tol)[0]), axis=0).shape[0] == 1
    assert {CR.relation_constants(config(n)[1])[2] for n in NAMES} == {1}
    dup = CC.cases()["subset_duplicate"][1]["indices"]
    assert np.unique(dup).size == dup.size - 1


@pytest.mark.parametrize("name", NAMES)
def test_partition_is_the_brute_force_components(name):
    cloud, tol, lo, hi, idx = config(name)
    _, _, clusters = CC.restated(name)
    label = CC.components(name)
    brute = CR.clusters_of_labels(label, lo, hi)
    assert sorted(map(tuple, map(sorted, clusters))) == sorted(map(tuple, map(sorted, brute)))
    # seeds ascend, so a cluster's first BFS element is its smallest position — the brute force's label
    for c in clusters:
        assert c[0] == min(c) == label[c[0]]
    assert CC.n_components(name) == np.unique(label).size


@pytest.mark.parametrize("name", NAMES)
def test_case_is_admitted(name):
    cloud, tol, _, _, idx = config(name)
    band, undecided = CR.admission(*cloud, tol, idx, cap=1e-5)
    assert undecided == 0, (band, undecided)
    if name in CC.DYADIC:
        assert band > 0  # `<=` decides, exactly


@pytest.mark.parametrize("name", NAMES)
def test_canonical_form_is_the_stable_order(name):
    cloud, tol, lo, hi, idx = config(name)
    ind, off, clusters = CC.restated(name)
    c_ind, c_off, c_lab = CC.answer(name)
    m = CC.list_length(name)
    # the same sizes in the same order: the restatement's sort is stable and its clusters exist in seed order
    assert np.array_equal(off, c_off)
    entries = np.arange(m, dtype=np.uint32) if idx is None else idx
    firsts = []
    for k, c in enumerate(clusters):
        got = c_ind[c_off[k]:c_off[k + 1]]
        assert np.array_equal(got, entries[np.asarray(sorted(c), dtype=np.int64)])  # the same cluster, positions ascending
        assert got[0] == entries[c[0]]                                               # its first element is the seed
        assert (c_lab[np.asarray(c, dtype=np.int64)] == k + 1).all()
        firsts.append(c[0])
    assert int((c_lab > 0).sum()) == c_ind.size
    for k in range(1, len(clusters)):  # equal sizes by smallest position
        if len(clusters[k]) == len(clusters[k - 1]):
            assert firsts[k] > firsts[k - 1]


# ------------------------------------------------------------------ wide keys, large lists ----
@pytest.mark.parametrize("name", sorted(CC.KEY_BITS))
def test_wide_cases_need_more_than_32_key_bits(name):
    cloud, tol, lo, hi, idx = config(name)
    bits, keys = CC.sort_keys(cloud, tol, idx)
    assert bits == CC.KEY_BITS[name] > 32
    # sensitivity: sorted by the low 32 bits alone (four radix passes) the keys are not in order — k_cluster_ranges
    # bisects them — and two occupied voxels share their low 32 bits
    by_low = np.argsort(keys & 0xFFFFFFFF, kind="stable")
    assert (np.diff(keys[by_low]) < 0).any()
    assert np.unique(keys & 0xFFFFFFFF).size < np.unique(keys).size
    vox = CR.voxels(CR._points(*cloud, idx)[0], CR.relation_constants(tol)[0])
    if name == "wide_corners":  # the accepted extremes, with clusters AT them
        assert vox.min() == CR.COORD_MIN + 1 and vox.max() == CR.COORD_MAX - 1
        assert (vox.min(axis=0) == CR.COORD_MIN + 1).all() and (vox.max(axis=0) == CR.COORD_MAX - 1).all()
        ind, off, _ = CC.restated(name)
        corner = {int(p) for p in np.nonzero((np.abs(vox) >= CR.COORD_MAX - 2).all(axis=1))[0]}
        assert sum(1 for k in range(off.size - 1) if set(ind[off[k]:off[k + 1]].tolist()) <= corner) >= 5
        assert 1 in sizes(off) and 40 in sizes(off)  # the singletons and the blob across two voxels


def test_blob_constructor_is_the_restatement_at_a_few_thousand_points():
    cloud, idx, blob = CL.blob_list(**CL.BLOBS_SMALL)
    assert 4000 <= idx.size <= 10000 and np.unique(idx).size < idx.size < cloud[0].size + idx.size
    assert CL.on_the_lattice(cloud, idx)
    pts, entries = CR._points(*cloud, idx)
    label = CR.components_brute(*cloud, CL.TOL, idx)
    for lo in (1, 10):
        clusters, comps = CR.cluster_core(pts, CL.TOL, lo, 100000)
        want = CR.canonical(clusters, entries, entries.size)
        got = CL.canonical_of_partition(blob, idx, lo, 100000)
        for a, b in zip(want, got[:3]):
            assert np.array_equal(a, b)
        assert got[3] == len(comps) == np.unique(label).size
        assert np.array_equal(CL.canonical_of_partition(label, idx, lo, 100000)[2], got[2])  # the brute force's partition
    # and the chain's constructor: one component by the BFS and by the brute force
    line = CL.chain_long(2049, 300)
    clusters, comps = CR.cluster_core(np.stack(line, axis=1), CL.TOL, 10, 100000)
    assert len(comps) == 1 and np.unique(CR.components_brute(*line, CL.TOL)).size == 1
    want = CR.canonical(clusters, np.arange(2049, dtype=np.uint32), 2049)
    got = CL.canonical_of_partition(np.zeros(2049), np.arange(2049, dtype=np.uint32), 10, 100000)
    assert all(np.array_equal(a, b) for a, b in zip(want, got[:3]))


def test_large_blob_cases_cross_what_they_were_built_for():
    cloud, idx, blob = CL.blobs_688k()
    m = idx.size
    assert m >= 655361 and m > CL.RS_SMALL_MAX and m > CL.INDEX_SWEEP and cloud[0].size < m
    assert np.unique(idx).size < m and int(idx.max()) < cloud[0].size and np.unique(idx).size < cloud[0].size
    assert CL.on_the_lattice(cloud, idx)  # admission, by construction
    # the partition is the construction's: blobs narrower than the tolerance, 1.6 or more apart
    pts, _ = CR._points(*cloud, idx)
    p64 = pts.astype(np.float64)
    order = np.argsort(blob, kind="stable")
    starts = np.nonzero(np.diff(blob[order], prepend=-1))[0]
    lo, hi = np.minimum.reduceat(p64[order], starts), np.maximum.reduceat(p64[order], starts)
    assert (np.linalg.norm(hi - lo, axis=1) < CL.TOL).all()
    centre = np.round((lo + hi) / 4.0) * 2.0
    assert np.unique(centre, axis=0).shape[0] == starts.size and (np.abs((lo + hi) / 2.0 - centre) < 0.2).all()
    for name, kept_positions, clusters in (("blobs_688k_min1", m, 161000), ("blobs_688k_min10", 300000, 25000)):
        ind, off, lab, comps = CL.answer(name)
        assert (ind.size, off.size - 1, comps) == (kept_positions, clusters, 161000)
        assert ind.size > CL.SCAN_CHUNK and clusters > 2 * 1024  # the ordered keys' run heads carry too
        assert int((lab > 0).sum()) == ind.size and off[-1] == ind.size
        # sensitivity: without the scan's carry the kept positions compact to another list, the run heads to other offsets
        if name.endswith("min10"):
            assert m - ind.size > CL.SCAN_CHUNK  # rejected by min_size
            assert ind.size <= CL.RS_SMALL_MAX < m  # the ordering sort takes the small tile in a histogram sized for m
        kept = np.nonzero(lab)[0].astype(np.uint32)
        if kept.size < m:
            assert not np.array_equal(SL.compact_without_carry(lab > 0), kept)
        heads = np.zeros(ind.size, dtype=bool)
        heads[off[:-1]] = True
        assert not np.array_equal(SL.compact_without_carry(heads), off[:-1])


def test_chain_case_is_one_component_over_a_thousand_blocks():
    (x, y, z), kw, _ = CL.cases()["chain_300k"]
    m = x.size
    assert m == CL.CHAIN > CL.SCAN_CHUNK and not y.any() and not z.any() and kw["max_size"] >= m
    sx = np.sort(x.astype(np.float64))
    assert (np.diff(sx) == 0.4375).all()  # a neighbour 0.875 tol away, the next one 1.75 tol: exact in fp32, no band
    a = np.stack([x[:2], y[:2], z[:2]], axis=1)
    dec = CR.decisions(np.zeros((2, 3), dtype=F), np.asarray([[0.4375, 0, 0], [0.875, 0, 0]], dtype=F), F(0.25))
    assert dec[:, 0].all() and not dec[:, 1].any() and a.shape == (2, 3)
    assert (np.abs(np.diff(x.astype(np.float64))) > 1.0).mean() > 0.99  # shuffled: list neighbours are far apart
    ind, off, lab, comps = CL.answer("chain_300k")
    assert comps == 1 and off.tolist() == [0, m] and np.array_equal(ind, np.arange(m)) and (lab == 1).all()
    # sensitivity: links that stay inside a block of 256 sorted points give ceil(m / 256) components, not one
    assert -(-m // 256) > 1024


# ------------------------------------------------------------------ the engine's host algebra, stand-alone and sanitized ----
PROBE = os.path.join(ROOT, "fastdem_amd", "cpp", "tests", "cluster_host_probe.cpp")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("cluster_host") / "cluster_host_probe")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "fastdem_amd", "csrc"), PROBE, "-o", exe])

    def run(*rows, expect=0):
        """Every row is one run of the probe; their outputs as lists of numbers."""
        out = []
        for numbers in rows:
            text = " ".join(float(v).hex() for v in numbers)
            r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
            assert r.returncode == expect, r.stdout[-2000:] + r.stderr[-4000:]
            out.append([float.fromhex(tok) for tok in r.stdout.split()])
        return out
    return run


def test_host_relation_constants_are_the_restatements(probe):
    rng = np.random.default_rng(13)
    tols = [0.5, 0.3, 0.1, 1.0, 0.05, 2.0, 1e-3, 100.0] + rng.uniform(0.05, 2.0, 40).astype(F).tolist()
    for tol, got in zip(tols, probe(*[(1, F(t)) for t in tols])):
        inv, r_sq, rng_ = CR.relation_constants(tol)
        assert got == [1.0, float(inv), float(r_sq), float(rng_)], (tol, got)
    refused = [0.0, -0.5, float("nan"), float("inf"), -float("inf"), 1e-45]  # (1 / 1e-45 overflows: no range)
    for tol, got in zip(refused, probe(*[(1, t) for t in refused])):
        assert got[0] == 0.0, tol


def test_host_key_layout(probe):
    bits = lambda v: max(int(v).bit_length(), 1)  # noqa: E731
    boxes = [((5, 5, 5), (5, 5, 5)), ((0, 0, 0), (2 ** 21 - 1, 2 ** 21 - 1, 2 ** 21 - 1)), ((100, 7, 1048576), (355, 8, 1048580)),
             ((1, 2, 3), (2, 4, 10))]
    for (lo, hi), got in zip(boxes, probe(*[(2, *lo, *hi, 1) for lo, hi in boxes])):
        ext = [h - l for l, h in zip(lo, hi)]
        assert got == [1.0, *map(float, ext), bits(ext[0]), bits(ext[1]), sum(bits(e) for e in ext)]
        assert got[-1] <= 63
    assert probe((2, 3, 0, 0, 2, 0, 0, 1))[0] == [0.0]             # an empty box
    assert probe((2, 0, 0, 0, 2 ** 21, 0, 0, 1))[0] == [0.0]        # a field beyond 21 bits
    # the key and back, at the corners and inside; keys keep the order (z, y, x)
    lo, hi = (100, 7, 1048576), (355, 8, 1048580)
    vs = [lo, hi, (101, 7, 1048576), (100, 8, 1048576), (100, 7, 1048577), (355, 8, 1048579), (200, 7, 1048578)]
    got = probe(*[(4, *lo, *hi, 1, *v) for v in vs])
    for v, g in zip(vs, got):
        assert g[1:] == list(map(float, v))
    order = sorted(range(len(vs)), key=lambda k: (vs[k][2], vs[k][1], vs[k][0]))
    assert order == sorted(range(len(vs)), key=lambda k: got[k][0])
    probe((4, *lo, *hi, 1, 99, 7, 1048576), expect=2)               # a voxel outside the box


def test_host_ordering_key_fits(probe):
    ms = [1, 2, 3, 255, 256, 257, 70000, 2 ** 31, 2 ** 32 - 4098]
    for m, got in zip(ms, probe(*[(3, m) for m in ms])):
        root_bits = max((m - 1).bit_length(), 1)
        assert got == [root_bits, 2 * root_bits] and got[1] <= 64
        # (m - size) << bits_root | root with size >= 1 and root <= m - 1 stays below 2^bits
        assert ((m - 1) << root_bits | (m - 1)) < 2 ** int(got[1])
