"""tests/post_cases.py on the CPU: the cases do what they are meant to (on the oracle alone), the kernel names they expect
are the launch sites of fdm_engine_post.inl, every one of them, and the thresholds restated there are the source's."""
import os
import re

import numpy as np
import pytest

import post_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastdem_amd", "csrc")
IDS = [c.id for c in PC.CASES]


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(src, name):
    m = re.search(r"\b%s\s*=\s*(\d+)u?\b" % re.escape(name), src)
    assert m, name
    return int(m.group(1))


# ---------------------------------------------------------------------------------------------- the source ----
def test_restated_constants_are_the_sources():
    hpp, inl = source("fdm_post.hpp"), source("fdm_engine_post.inl")
    assert constant(hpp, "kMaxRegion") == PC.K_MAX_REGION
    assert (constant(hpp, "kS3R_"), constant(hpp, "kS3C_")) == (PC.S3R, PC.S3C)
    assert constant(hpp, "kFusionWaveMax") == PC.FUSION_WAVE_MAX
    assert constant(hpp, "kFusHaloMax") == PC.FUS_HALO_MAX
    assert constant(hpp, "kFeatHaloMax") == PC.FEAT_HALO_MAX
    assert (constant(hpp, "kFeatTileR"), constant(hpp, "kFeatTileC")) == PC.FEAT_TILE
    # both selection kernels are held to the same 160 KB, spelled `160u * 1024u`, and nothing else is
    caps = re.findall(r"(\w+_lds_bytes)\([^;{]*?\)\s*<=\s*(\d+)u \* (\d+)u", inl)
    assert sorted(c[0] for c in caps) == ["features_sel_lds_bytes", "median_sel_lds_bytes"]
    assert all(int(a) * int(b) == PC.LDS_CAP for _, a, b in caps)
    assert re.search(r"std::min<size_t>\(\(\(e->ncell \+ threads - 1\) / threads\) \* threads, (\d+)\)", inl).group(1) == \
        str(PC.POOL_THREADS)
    # the formulas themselves, as text
    assert "unsigned(kS3R_ + 2 * (kernel / 2)) * unsigned(kS3C_ + 2 * (kernel / 2)) * 4u" in hpp
    assert "unsigned(kS3R_ + 2 * halo) * unsigned(kS3C_ + 2 * halo) * 8u + unsigned(n_entries) * 4u" in hpp
    assert "static_cast<int>(lo_pct * float(nmax - 1)) + 1" in inl
    assert "(nmax - 1) - static_cast<int>(hi_pct * float(nmax - 1)) + 1" in inl
    assert "if (d2 <= r2 * (1.0f + 1e-5f)) reg.push_back" in inl and "std::floor(radius / res + 1e-4f)" in inl


def test_thresholds():
    assert PC.MEDIAN_SEL_MAX == 183 and PC.median_sel_lds_bytes(183) == 162640 <= PC.LDS_CAP < PC.median_sel_lds_bytes(184)
    assert PC.median_kernel(15) == PC.median_kernel(14) == "k_median" and PC.median_kernel(16) == "k_median_sel"
    assert PC.FEATURES_SEL_REACH == 53
    n_sel = PC.region_disc(PC.cells(PC.FEATURES_SEL_RADIUS))[0].size
    n_big = PC.region_disc(PC.cells(PC.FEATURES_BIG_RADIUS))[0].size
    assert PC.reach(PC.cells(PC.FEATURES_SEL_RADIUS)) == 53 and PC.reach(PC.cells(PC.FEATURES_BIG_RADIUS)) == 54
    assert PC.features_sel_lds_bytes(53, n_sel) <= PC.LDS_CAP < PC.features_sel_lds_bytes(54, n_big)
    assert PC.features_sel_lds_bytes(53, n_sel) > 0.99 * PC.LDS_CAP      # the granted maximum, within 1 %
    for c, (n, n_pad) in PC.FUSION_DISCS.items():
        assert PC.region_disc(PC.cells(c))[0].size == n, c
        assert (PC.fusion_n_pad(n) if n <= PC.FUSION_WAVE_MAX else None) == n_pad, c
        again = PC.region_disc(PC.cells(PC.FUSION_AGAIN[c]))[0].size
        assert again != n and (again > PC.FUSION_WAVE_MAX) == (n > PC.FUSION_WAVE_MAX)
    assert sorted(v[1] for v in PC.FUSION_DISCS.values() if v[1]) == [64, 128, 256, 512, 1024]
    assert [PC.region_disc(PC.cells(c))[0].size for c in (7, 8, 9, 15)] == [149, 197, 253, 709]
    assert PC.region_disc(PC.cells(9))[0].size <= PC.K_MAX_REGION < PC.region_disc(PC.cells(9.5))[0].size
    assert PC.need_lo_hi(709, 0.0, 1.0) == (1, 1)
    lo, hi = PC.need_lo_hi(709, 0.015, 0.985)
    assert 9 <= lo <= 16 and 9 <= hi <= 16


def test_no_region_within_kmaxregion_exceeds_the_lds_of_features_sel():
    """The feature dispatch has no arm between k_features_sel and k_features_big: every disc of at most kMaxRegion cells
    fits the LDS of k_features_sel (the static_assert beside the dispatch states the same with its bound of 11 cells)."""
    seen = set()
    for hundredths in range(0, 1301):             # radii of 0 .. 13 cells: the disc of 9.06 cells is the first beyond 256
        radius = PC.cells(hundredths / 100.0)
        n, halo = PC.region_disc(radius)[0].size, PC.reach(radius)
        if n <= PC.K_MAX_REGION:
            seen.add((halo, n))
            assert halo <= 11 and PC.features_sel_lds_bytes(halo, n) <= PC.LDS_CAP, (hundredths, halo, n)
        else:
            assert hundredths > 900, hundredths       # (the count only grows with the radius)
    assert max(n for _, n in seen) == 253 and max(h for h, _ in seen) == 9
    assert PC.features_sel_lds_bytes(11, PC.K_MAX_REGION) <= PC.LDS_CAP
    inl = source("fdm_engine_post.inl")
    assert "160u * 1024u >= features_sel_lds_bytes(11, kMaxRegion)" in inl and "kMaxRegion < 17 * 17" in inl


def recorded_names():
    """Every name a launch site of the four stages records: the argument of FDM_POST_KERNEL(...)."""
    inl = source("fdm_engine_post.inl")
    body = inl[inl.index("int fdm_engine_apply_inpainting"):]
    names = re.findall(r"FDM_POST_KERNEL\(((?:[^()<>]|<[^<>]*>)+)\)", body)
    assert names
    # every launch of a stage kernel goes through the macro (k_copy_strided2 is a staging copy, not a stage kernel)
    bare = re.findall(r"hipLaunchKernelGGL\(\s*(k_\w+)", body)
    assert set(bare) <= {"k_copy_strided2"}, bare
    for helper in ("launch_f64", "launch_tiled", "launch_feat"):
        calls = re.findall(r"\b%s\(([^;]*)\);" % helper, body)
        assert calls and all(c.startswith("FDM_POST_KERNEL(") for c in calls), (helper, calls)
    return set(" ".join(n.split()) for n in names)


def asserted_in_test_post_gpu():
    with open(os.path.join(ROOT, "tests", "test_post_gpu.py")) as f:
        txt = f.read()
    return set(re.findall(r"\"(k_[a-z0-9_]+(?:<[0-9a-z, ]+>)?)\"", txt))


def test_every_launch_site_is_expected_by_a_test():
    """parsed launch sites == names of the case table + names asserted in test_post_gpu.py: a launch site added without
    a test fails here, and so does a test that expects a name no site records."""
    sites = recorded_names()
    expected = {c.kernel for c in PC.CASES if c.kernel} | asserted_in_test_post_gpu()
    assert sites == expected, (sorted(sites - expected), sorted(expected - sites))
    # and the table alone reaches what no test ran before it
    table = {c.kernel for c in PC.CASES}
    assert {"k_median_big", "k_fusion_big", "k_features_big", "k_features<8>", "k_features<16>", "k_fusion_wave",
            "k_median_sel", "k_features_sel", "k_features_tiled<16>", ""} <= table


def test_table_names_are_what_the_restated_dispatch_gives():
    assert len(set(IDS)) == len(IDS)
    for c in PC.CASES:
        assert PC.kernel_of(c.stage, c.params) == c.kernel, c.id
        if c.kernel in PC.POOLED:     # the third call runs the pool at a second size
            assert PC.kernel_of(c.stage, c.again) == c.kernel and c.again[0] != c.params[0], c.id
    # the grid-stride cases: more cells than threads in flight, and nowhere else
    for c in PC.CASES:
        if c.map == "grid":
            assert c.kernel in PC.POOLED and PC.MAPS["grid"][2] * PC.MAPS["grid"][3] > PC.POOL_THREADS
    assert {c.kernel for c in PC.CASES if c.map == "grid"} == {"k_fusion_big", "k_features_big"}
    # every n_pad at every quantile pair, and a split
    for tag in ("wave64", "wave128", "wave256", "wave512", "wave1024", "big"):
        ids = [i for i in IDS if i.startswith("fusion-%s-" % tag)]
        assert len([i for i in ids if "-q" in i]) >= len(PC.QUANTILES) and "fusion-%s-split" % tag in ids


def test_pooled_cases_stay_under_the_cost_bound():
    pooled = [c for c in PC.CASES if c.kernel in PC.POOLED]
    assert pooled
    for c in pooled:
        assert PC.list_moves(c) <= PC.MAX_LIST_MOVES, (c.id, PC.list_moves(c))


def test_grid_stride_cases_give_a_thread_two_finite_cells():
    for c in PC.CASES:
        if c.map != "grid":
            continue
        ok = np.ones(PC.MAPS["grid"][2:4], dtype=bool)
        for a in PC.field(c.field, c.map).values():
            ok &= np.isfinite(a)
        order = ok.ravel(order="F")            # t = column * rows + row
        both = order[:order.size - PC.POOL_THREADS] & order[PC.POOL_THREADS:]
        assert both.sum() >= 3, (c.id, int(both.sum()))
    sparse = np.isfinite(PC.field("elevation_sparse", "grid")["elevation"])
    assert 0.02 <= sparse.mean() <= 0.04


# ---------------------------------------------------------------------------------------------- the oracle ----
def test_maps_have_the_shapes_the_cases_assume(R):
    for name, (w, h, rows, cols, shift) in PC.MAPS.items():
        m = R.RefEngine(w, h, PC.RES)
        moved = m.move(*shift)
        assert (m.rows, m.cols) == (rows, cols), name
        assert moved[0] % rows and moved[1] % cols, name     # the seam is inside the map
    rows, cols = PC.MAPS["small"][2:4]
    assert all(rows % k and cols % k for k in (4, 8, 16, 32))
    assert PC.MAPS["strip"][2] < min(PC.S3C, PC.FEAT_TILE[1])
    assert PC.MAPS["grid"][2] * PC.MAPS["grid"][3] > PC.POOL_THREADS
    # the tall map is longer than the reach of the largest windows tested: they are not the whole map for every cell
    assert PC.MAPS["tall"][2] > (PC.MEDIAN_SEL_MAX + 1) // 2 and PC.MAPS["tall"][2] > PC.FEATURES_SEL_REACH + 1


def run_oracle(R, case, params):
    """(layers before, layers after) of the case's call on the oracle; a layer the call creates is NaN before."""
    w, h = PC.MAPS[case.map][:2]
    m = R.RefEngine(w, h, PC.RES)
    m.move(*PC.MAPS[case.map][4])
    PC.set_layers(m, case)
    names = PC.OUTPUTS[case.stage]
    before = {n: m.layer(n) if m.exists(n) else None for n in names}
    R.set_trig_mode(1)
    try:
        PC.apply(m, case.stage, params)
    finally:
        R.set_trig_mode(0)
    after = {n: m.layer(n) for n in names if m.exists(n)}
    return before, after


def changed_share(case, params, before, after):
    """Share of the cells the stage works on (a finite centre; for inpainting the empty cells it may fill) in which some
    output layer differs from what it held."""
    lay = PC.field(case.field, case.map)
    centre = np.ones(PC.MAPS[case.map][2:4], dtype=bool)
    for a in lay.values():
        centre &= np.isfinite(a)
    if case.stage == "inpaint":
        out = after["elevation" if params[2] else "elevation_inpainted"]
        return (np.isfinite(out) & ~centre).sum() / max(1, (~centre).sum())
    diff = np.zeros(centre.shape, dtype=bool)
    for n, a in after.items():
        b = before[n] if before[n] is not None else np.full(a.shape, np.nan, dtype=a.dtype)
        diff |= ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not (diff & ~centre).any(), case.id                # a cell without a finite centre is never written
    return (diff & centre).sum() / centre.sum()


@pytest.mark.parametrize("case", PC.CASES, ids=IDS)
def test_case_is_admitted(R, case):
    """The stage changes at least 10 % of the cells it works on — in the first call and in the changed one — and a
    `min_valid` chosen to split them leaves between 10 % and 90 % written: both outcomes occur."""
    for params in (case.params, case.again):
        if case.stage == "inpaint" and params[0] == 0:
            continue
        share = changed_share(case, params, *run_oracle(R, case, params))
        assert share >= 0.10, (case.id, params, share)
        if case.split:
            assert 0.10 <= share <= 0.90, (case.id, params, share)


FUSION_FIELDS = sorted({(c.map, c.field, round(c.params[0] / PC.RES, 3)) for c in PC.CASES if c.stage == "fusion" and c.map != "grid"})


@pytest.mark.parametrize("map_name,field_name,cells", FUSION_FIELDS)
def test_adversarial_field_puts_every_trap_into_one_neighbourhood(map_name, field_name, cells):
    """Counted from the field and the region: some cell with finite bounds has, inside its disc and among the cells
    with finite bounds, two equal samples (a tie), a -0.0, a pair whose weight is <= 1e-6 and an inverted pair."""
    lay = PC.field(field_name, map_name)
    up, lo = lay["upper_bound"], lay["lower_bound"]
    ok = np.isfinite(up) & np.isfinite(lo)
    radius = PC.cells(cells)
    with np.errstate(invalid="ignore", divide="ignore"):
        weight = (np.float32(1.0) / ((up - lo) + np.float32(1e-4))).astype(np.float32)   # the spatial factor is <= 1
    taken = ok & (weight > np.float32(1e-6))
    plateau = taken & (up == np.float32(0.25)) & (lo == np.float32(-0.125))
    neg_zero = taken & (((lo == 0) & np.signbit(lo)) | ((up == 0) & np.signbit(up)))
    pos_zero = taken & (((lo == 0) & ~np.signbit(lo)) | ((up == 0) & ~np.signbit(up)))
    dropped = ok & (weight <= np.float32(1e-6)) & (weight >= 0)
    inverted = ok & (up < lo)
    n = {k: PC.neighbour_counts(v, radius) for k, v in
         dict(plateau=plateau, neg_zero=neg_zero, pos_zero=pos_zero, dropped=dropped, inverted=inverted).items()}
    every = ok & (n["plateau"] >= 2) & (n["neg_zero"] >= 1) & (n["pos_zero"] >= 1) & (n["dropped"] >= 1) & (n["inverted"] >= 1)
    assert every.sum() >= 1, {k: int((v > 0).sum()) for k, v in n.items()}
