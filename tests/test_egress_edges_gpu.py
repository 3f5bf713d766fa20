"""Map egress of the HIP engine (fdm_egress.hpp, the pack half of fdm_engine_io.inl) on the edges of its kernels:
count per 256-thread block -> k_pack_scan (one block, carry across 1024-entry chunks) -> ranked write through LDS.

Every pack is compared on the uint32 view of its records, EXACTLY, with the field list, point_step and point count,
against two independent readings of toPointCloud2Impl (bridge/ros/impl.hpp:28-166): the NumPy restatement
(tests/io_restate.py) and, where it supports the case, the oracle.  The inputs are tests/io_cases.py's, which
tests/test_io_restate_vs_oracle.py has already run through both readings on the CPU."""
import ctypes as C

import numpy as np
import pytest

import io_cases as K
from helpers import assert_layers_bit_identical, pair, run_both, same_geometry
from io_restate import restate_pack

pytestmark = pytest.mark.gpu
F32 = np.float32


# ------------------------------------------------------------------------------------------------------ helpers ----
def make_eng(gpu, tile=None):
    def make(width, height, res, fill_cfg, position):
        return gpu.Engine(width, height, res, fill_cfg(gpu.capi.default_config()), position=position, tile=tile)
    return make


_oracle = {}


def oracle_packs(R, case):
    """{sub: (fields, step, records)} of the oracle, computed once per case."""
    if case.name not in _oracle:
        ref, _ = case.create(lambda w, h, res, fill, pos: R.RefEngine(w, h, res, fill(R.default_config()), position=pos))
        _oracle[case.name] = {sub: ref.pack_cloud(case.elevation_layer, sub) for sub in case.subs}
        ref.close()
    return _oracle[case.name]


def same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ug, uw = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert np.array_equal(ug, uw), f"{what}: {int((ug != uw).sum())} words differ, first at {np.argwhere(ug != uw)[0]}"


def layers_of(eng, written=None):
    layers = {n: eng.layer(n) for n in eng.layers()}
    for n, a in (written or {}).items():   # what the test uploaded is what the engine holds, and what is restated
        same_bits(layers[n], a, n)
        layers[n] = a
    return layers


def check_case(eng, case, written, oracle=None, window=None):
    layers = layers_of(eng, written)
    order, geo = eng.layers(), eng.geometry()
    for sub in case.subs:
        fields, step, data = eng.pack_cloud(case.elevation_layer, sub)
        want_fields, want = restate_pack(layers, order, geo, case.elevation_layer, sub, window)
        assert fields == want_fields and step == 4 * len(want_fields), (case, sub)
        same_bits(data, want, (case, sub, "restatement"))
        if case.fields is not None:
            assert len(fields) == case.fields
        if oracle is not None:
            f_ref, s_ref, d_ref = oracle[sub]
            assert fields == f_ref and step == s_ref, (case, sub)
            same_bits(data, d_ref, (case, sub, "oracle"))
    # the map is read, never written
    assert same_geometry(eng.geometry(), geo)
    after = layers_of(eng)
    for n in order:
        same_bits(after[n], layers[n], n)


def raw_pack(gpu, eng, layer=b"elevation", sub=(0, 0, -1, -1), out=None, cap=0, names=None, names_cap=0):
    """fdm_engine_pack_cloud as a C caller sees it: (rc, n_points, point_step)."""
    n, step = C.c_uint64(0), C.c_uint32(0)
    rc = gpu.capi.load().fdm_engine_pack_cloud(eng._h, layer, *sub, None if out is None else out.ctypes.data_as(C.c_void_p),
                                               cap, C.byref(n), C.byref(step), names, names_cap)
    return rc, n.value, step.value


# -------------------------------------------------------------------------------------------------- the case table ----
@pytest.mark.parametrize("case", K.EGRESS_CASES, ids=repr)
def test_pack_on_the_edges(gpu, R, case):
    """Record widths 10 / 63 / 64 / 65 / 67 / 68 fields (the write kernel's LDS crosses 64 KB at 64), cell counts
    1 / 255 / 256 / 257, the scan's chunk edge at 262 143 / 262 144 / 262 656 cells, validity patterns that leave
    blocks and waves empty or full, submaps of a moved map, both estimators, other elevation layers, a far-off map."""
    eng, written = case.create(make_eng(gpu))
    check_case(eng, case, written, oracle_packs(R, case))
    eng.close()


@pytest.mark.parametrize("case", K.EGRESS_ENGINE_ONLY, ids=repr)
def test_pack_of_per_layer_storage(gpu, R, case):
    """Option records=0: one array per layer instead of cell records — another stride for every estimator layer."""
    eng, written = case.create(make_eng(gpu))
    twin = next(c for c in K.EGRESS_CASES if c.name == case.name.replace("per_layer", "records"))
    check_case(eng, case, written, oracle_packs(R, twin))
    eng.close()


def test_one_field_too_many_is_refused(gpu):
    """64 float layers fill a record (67 fields, 68 with rgb: include/fdm_engine.h); the 65th is FDM_ERR_INVALID, and
    neither the map nor the caller's buffer from the pack before is touched."""
    widest = next(c for c in K.EGRESS_CASES if c.name == "fields_67")
    eng, written = widest.create(make_eng(gpu))
    rc, n, step = raw_pack(gpu, eng)
    assert (rc, step) == (0, 67 * 4) and n > 0
    out = np.full(n * step + 64, 0xAB, dtype=np.uint8)
    assert raw_pack(gpu, eng, out=out, cap=n * step) == (0, n, step)
    earlier = out.copy()
    assert (earlier[n * step:] == 0xAB).all() and (earlier[:n * step] != 0xAB).any()
    eng.add("one_more", 0.5)
    before, geo = layers_of(eng), eng.geometry()
    names = C.create_string_buffer(4096)
    rc, _, _ = raw_pack(gpu, eng, out=out, cap=out.size, names=names, names_cap=4096)
    assert rc == gpu.capi.FDM_ERR_INVALID
    assert np.array_equal(out, earlier)
    d = C.c_void_p()
    n64 = C.c_uint64(0)
    assert gpu.capi.load().fdm_engine_pack_cloud_device(eng._h, b"elevation", 0, 0, -1, -1, C.byref(d), C.byref(n64),
                                                        None) == gpu.capi.FDM_ERR_INVALID
    with pytest.raises(gpu.EngineError):
        eng.pack_cloud()
    after = layers_of(eng)
    assert list(after) == list(before) and same_geometry(eng.geometry(), geo)
    for name in before:
        same_bits(after[name], before[name], name)
    # the same 65 float layers built in one go (tests/io_cases.py EGRESS_TOO_WIDE)
    eng2, _ = K.EGRESS_TOO_WIDE.create(make_eng(gpu))
    assert raw_pack(gpu, eng2)[0] == gpu.capi.FDM_ERR_INVALID
    assert raw_pack(gpu, eng2, layer=b"elevation_min")[0] == gpu.capi.FDM_ERR_INVALID
    eng.close()
    eng2.close()


def test_map_takes_128_layers_and_refuses_the_next(gpu):
    """The map's own cap (include/fdm_engine.h) lies well above the widest record, so that every record width up to
    the pack's cap can be reached whatever the estimator keeps internally; one layer more is FDM_ERR_INVALID and
    leaves the layer list as it was."""
    eng = gpu.Engine(0.5, 0.5, 0.5, gpu.capi.default_config())
    k = 0
    while len(eng.layers()) < 128:
        eng.add("u%03d" % k, float(k))
        k += 1
    names = eng.layers()
    with pytest.raises(gpu.EngineError):
        eng.add("one_more", 0.0)
    assert eng.layers() == names and not eng.exists("one_more")
    assert eng.layer("u%03d" % (k - 1))[0, 0] == float(k - 1)
    eng.add("u000", 7.0)     # adding an existing layer overwrites it, also on a full map
    assert eng.layer("u000")[0, 0] == 7.0
    with pytest.raises(gpu.EngineError):
        eng.pack_cloud()     # far more than 64 float layers
    eng.close()


def test_submaps_outside_the_buffer_are_refused(gpu):
    case = next(c for c in K.EGRESS_CASES if c.name == "submaps_moved")
    eng, _ = case.create(make_eng(gpu))
    g = eng.geometry()
    assert (g.rows, g.cols) == (24, 18) and (g.start_row, g.start_col) != (0, 0)
    out = np.full(24 * 18 * 40 + 64, 0xAB, dtype=np.uint8)
    for sub in K.BAD_SUBMAPS_24x18:
        rc, _, _ = raw_pack(gpu, eng, sub=sub, out=out, cap=out.size)
        assert rc == gpu.capi.FDM_ERR_INVALID, sub
        assert (out == 0xAB).all(), sub
    eng.close()


def test_tiled_engine_packs_its_window(gpu):
    """A tiled engine stores a window of the buffer and skips the cells outside it: a whole-buffer pack and submaps
    that straddle the window's edges (one of them wrapping around the buffer) yield the window's cells only, in the
    reference's order."""
    cfg = gpu.capi.default_config()
    cfg.mode = 1
    tile = (32, 64, 100, 70, 40, 70, 80, 60)   # stored 100 x 70 window of a 200 x 160 buffer
    eng = gpu.Engine(20.0, 16.0, 0.1, cfg, tile=tile)
    assert (eng.s_rows, eng.s_cols) == (100, 70) and (eng.rows, eng.cols) == (200, 160)
    rng = np.random.default_rng(9)
    written = {"elevation": np.asfortranarray(K.holes(rng, 100, 70, 0.3)),
               "variance": np.asfortranarray(K.wild(rng, 100, 70))}
    for name, a in written.items():
        eng.set_layer(name, a)
    case = K.MapCase("tiled", 200, 160, res=0.1,
                     subs=[None, (20, 50, 30, 40), (190, 120, 60, 30), (131, 133, 5, 5), (0, 0, 32, 160)])
    check_case(eng, case, written, window=tile[:4])
    n_sub = [eng.pack_cloud(sub=s)[2].shape[0] for s in case.subs]
    assert n_sub[0] == int(np.isfinite(written["elevation"]).sum()) and n_sub[1] > 0 and n_sub[2] > 0
    assert n_sub[3] <= 1 and n_sub[4] == 0     # the window's last cell alone; a strip that misses the window
    eng.close()


# -------------------------------------------------------------------------------------------------- C ABI contract ----
def test_size_query_and_short_buffer_write_nothing(gpu):
    case = next(c for c in K.EGRESS_CASES if c.name == "fields_natural")
    eng, written = case.create(make_eng(gpu))
    fields, want = restate_pack(layers_of(eng, written), eng.layers(), eng.geometry())
    n_want, step_want = want.shape[0], 4 * len(fields)
    size = n_want * step_want
    assert raw_pack(gpu, eng) == (0, n_want, step_want)                      # host_out == NULL
    guard = 32
    buf = np.full(size + 2 * guard, 0xCD, dtype=np.uint8)
    inner = buf[guard:guard + size]
    assert raw_pack(gpu, eng, out=inner, cap=size - 1) == (0, n_want, step_want)   # one byte short
    assert (buf == 0xCD).all()
    assert raw_pack(gpu, eng, out=inner, cap=size) == (0, n_want, step_want)       # exactly enough
    assert (buf[:guard] == 0xCD).all() and (buf[guard + size:] == 0xCD).all()
    same_bits(inner.view(F32).reshape(n_want, -1), want, "records between the guards")
    eng.close()


def test_field_names_are_truncated_inside_the_buffer(gpu):
    case = next(c for c in K.EGRESS_CASES if c.name == "fields_natural")
    eng, _ = case.create(make_eng(gpu))
    joined = "\n".join(eng.pack_cloud()[0]).encode()
    assert len(joined) > 40
    for cap in (1, 2, 10, len(joined), len(joined) + 1):
        names = C.create_string_buffer(b"\x7f" * 256, 256)
        assert raw_pack(gpu, eng, names=names, names_cap=cap)[0] == 0
        raw = names.raw
        kept = min(cap - 1, len(joined))
        assert raw[:kept] == joined[:kept] and raw[kept] == 0, cap
        assert raw[max(cap, kept + 1):] == b"\x7f" * (256 - max(cap, kept + 1)), cap
    # the Python handle with a caller-sized names buffer
    assert "\n".join(eng.pack_cloud(names_cap=len(joined) + 1)[0]).encode() == joined
    eng.close()


def test_second_smaller_pack_reuses_the_device_buffer(gpu):
    case = next(c for c in K.EGRESS_CASES if c.name == "fields_67")
    sub = (18, 11, 7, 6)
    a, _ = case.create(make_eng(gpu))
    _, _, big = a.pack_cloud()
    f2, s2, second = a.pack_cloud(sub=sub)
    b, _ = case.create(make_eng(gpu))
    f1, s1, fresh = b.pack_cloud(sub=sub)
    assert 0 < fresh.shape[0] < big.shape[0] and (f1, s1) == (f2, s2)
    same_bits(second, fresh, "second pack")
    _, want = restate_pack(layers_of(b), b.layers(), b.geometry(), sub=sub)
    same_bits(second, want, "second pack vs restatement")
    a.close()
    b.close()


def T(x=0.0, y=0.0, z=0.0):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def small_scan(seed, n=2500):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.4, 2.2, n).astype(F32)   # (a strip of the map stays unobserved)
    y = rng.uniform(-2.6, 2.6, n).astype(F32)
    z = (0.3 * np.sin(0.9 * x) * np.cos(0.7 * y) - 0.6 + 0.01 * rng.standard_normal(n)).astype(F32)
    return {"x": x, "y": y, "z": z, "intensity": None, "rgb": None}


def test_pack_between_two_scans_of_a_stream(gpu, R):
    """A scan enqueued on the device leaves its update held back; a pack in between launches it first and shows that
    scan; the stream then goes on bit-identical to the oracle."""
    import torch

    def fill(c):
        c.mode = 0
    eng, ref = pair(gpu, R, 6.4, 4.8, 0.1, fill)
    Tbs = T(z=0.6)
    run_both(eng, ref, small_scan(20), Tbs, T())
    s = small_scan(21)
    d = {k: torch.from_numpy(s[k]).cuda() for k in ("x", "y", "z")}
    eng.integrate_device(d["x"], d["y"], d["z"], Tbs, T(0.31, 0.22))
    rc, _ = ref.integrate(s["x"], s["y"], s["z"], Tbs, T(0.31, 0.22))
    assert rc == 0
    fields, step, data = eng.pack_cloud()
    f_ref, s_ref, d_ref = ref.pack_cloud()
    assert fields == f_ref and step == s_ref and d_ref.shape[0] > 500
    same_bits(data, d_ref, "oracle")
    _, want = restate_pack({n: ref.layer(n) for n in ref.layers()}, ref.layers(), ref.geometry())
    same_bits(data, want, "restatement of the oracle's map")
    run_both(eng, ref, small_scan(22), Tbs, T(0.5, 0.5))
    assert_layers_bit_identical(eng, ref)
    assert same_geometry(eng.geometry(), ref.geometry())
    eng.close()
