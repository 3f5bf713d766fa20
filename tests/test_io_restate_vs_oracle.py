"""The NumPy restatements of map egress and PointCloud2 ingest (tests/io_restate.py, written from the reference's
source) against the oracle (oracle/fdm_ref_egress.hpp, fdm_ref_ingest.hpp), on every input the GPU edge tests use
(tests/io_cases.py).  Two independent readings of the reference that must agree bit for bit before either is used to
judge the engine; where they differ the reference's source decides which side is wrong.  Runs without a GPU."""
import numpy as np
import pytest

import io_cases as K
from io_restate import restate_from_cloud2, restate_pack

F32 = np.float32


def make_ref(R):
    def make(width, height, res, fill_cfg, position):
        return R.RefEngine(width, height, res, fill_cfg(R.default_config()), position=position)
    return make


def same_records(got, want, what):
    (fg, dg), (fw, dw) = got, want
    assert fg == fw, what
    assert dg.shape == dw.shape, (what, dg.shape, dw.shape)
    ug, uw = np.ascontiguousarray(dg).view(np.uint32), np.ascontiguousarray(dw).view(np.uint32)
    assert np.array_equal(ug, uw), f"{what}: {int((ug != uw).sum())} words differ, first at {np.argwhere(ug != uw)[0]}"


@pytest.mark.parametrize("case", K.EGRESS_CASES + [K.EGRESS_TOO_WIDE], ids=repr)
def test_pack_restatement_equals_oracle(R, case):
    ref, written = case.create(make_ref(R))
    layers = {n: ref.layer(n) for n in ref.layers()}
    for n, a in written.items():      # the restatement reads what the test wrote, not what the oracle made of it
        assert np.array_equal(layers[n].view(np.uint32), a.view(np.uint32)), n
        layers[n] = a
    for sub in case.subs:
        fields, step, data = ref.pack_cloud(case.elevation_layer, sub)
        assert step == 4 * len(fields)
        if case.fields is not None:
            assert len(fields) == case.fields
        same_records((fields, data), restate_pack(layers, ref.layers(), ref.geometry(), case.elevation_layer, sub),
                     (case, sub))
    ref.close()


def test_pack_restatement_on_a_hand_made_map():
    """Known answers, independent of the oracle: 4 x 3 cells of 0.5 m around the origin, start index (1, 2)."""
    class G:
        rows, cols, start_row, start_col = 4, 3, 1, 2
        position_x, position_y, length_x, length_y, resolution = 0.0, 0.0, 2.0, 1.5, 0.5
    el = np.full((4, 3), np.nan, F32)
    el[1, 2], el[0, 2], el[1, 0], el[3, 1] = 1.0, 2.0, 3.0, np.inf
    other = np.arange(12, dtype=F32).reshape(4, 3)
    col = np.full((4, 3), 7, np.uint32).view(F32)
    fields, d = restate_pack({"elevation": el, "_hidden": other, "w": other, "color": col},
                             ["elevation", "_hidden", "color", "w"], G)
    assert fields == ["x", "y", "z", "w", "rgb"]
    # visiting order: column 2 first (rows 1, 2, 3, 0), then column 0; the start cell is the map's +x +y corner
    assert np.array_equal(d[:, :4], np.array([[0.75, 0.5, 1.0, 5.0], [-0.75, 0.5, 2.0, 2.0], [0.75, 0.0, 3.0, 3.0]], F32))
    assert (d[:, 4].view(np.uint32) == 7).all()
    # a 2 x 2 submap from buffer cell (0, 2): rows 0, 1 and columns 2, 0
    _, s = restate_pack({"elevation": el}, ["elevation"], G, sub=(0, 2, 2, 2))
    assert np.array_equal(s, np.array([[-0.75, 0.5, 2.0], [0.75, 0.5, 1.0], [0.75, 0.0, 3.0]], F32))
    # a stored window of rows 1..2, columns 0..1: only (1, 0) is inside and finite
    _, w = restate_pack({"elevation": el[1:3, 0:2].copy()}, ["elevation"], G, window=(1, 0, 2, 2))
    assert np.array_equal(w, np.array([[0.75, 0.0, 3.0]], F32))


@pytest.mark.parametrize("name", list(K.INGEST_CASES))
def test_from_cloud2_restatement_equals_oracle(R, name):
    blob, lay, n, _ = K.ingest_case(name)
    got, want = restate_from_cloud2(blob, n, lay), R.from_cloud2(blob, n, lay)
    for k in ("x", "y", "z", "intensity", "rgb"):
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    if name.startswith("type_"):
        assert got["intensity"].size and not got["intensity"].view(np.uint32).any()


def test_float64_intensities_round_once_to_nearest_even():
    """Known answers for static_cast<float>(double), independent of the oracle."""
    x = np.ones(K.F64_VALUES.size, F32)
    from cloud2 import make_blob
    blob, lay = make_blob(x, x, x, intensity=K.F64_VALUES, intensity_type=8)
    got = restate_from_cloud2(blob, x.size, lay)["intensity"]
    want = {1e300: np.inf, -1e300: -np.inf, 1e-320: 0.0, 1e-46: 0.0, 2.0 ** -149: 2.0 ** -149, 2.0 ** -150: 0.0,
            1.5 * 2.0 ** -149: 2.0 ** -148, 2.5 * 2.0 ** -149: 2.0 ** -148, 1 + 2.0 ** -24: 1.0,
            1 + 3 * 2.0 ** -24: 1 + 2.0 ** -22, 1 + 2.0 ** -24 + 2.0 ** -50: 1 + 2.0 ** -23,
            K.FLT_MAX * (1 + 2.0 ** -25): K.FLT_MAX, K.FLT_MAX * (1 + 2.0 ** -24): np.inf}
    for v, f in want.items():
        k = int(np.flatnonzero(K.F64_VALUES == v)[0])
        assert got[k] == F32(f) and np.signbit(got[k]) == np.signbit(F32(f)), (v, got[k], f)
    assert np.isnan(got[np.isnan(K.F64_VALUES)]).all()
    assert np.signbit(got[np.flatnonzero(K.F64_VALUES == 0.0)]).tolist() == [False, True]
