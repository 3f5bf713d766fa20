"""PointCloud2 ingest of the HIP engine (fdm_ingest.hpp) on the edges of its kernels: count per 256-thread block ->
k_pack_scan (shared with egress; carry across 1024-entry chunks) -> ranked write.

The decoded channels are compared bit for bit, in message order, with two independent readings of nanopcl's from_impl
(nanopcl/bridge/ros/impl.hpp:104-119, 169-177, 179-270): the NumPy restatement (tests/io_restate.py) and the oracle.
The inputs are tests/io_cases.py's, which tests/test_io_restate_vs_oracle.py has already run through both readings on
the CPU."""
import numpy as np
import pytest

import io_cases as K
from helpers import assert_layers_equal, lay_of, pair
from io_restate import restate_from_cloud2, restate_pack

pytestmark = pytest.mark.gpu
F32 = np.float32
CHANNELS = ("x", "y", "z", "intensity", "rgb")


def same_channels(got, want, what):
    for k in CHANNELS:
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, \
            (what, k, None if got[k] is None else got[k].shape, want[k].shape)
        ug, uw = got[k].view(np.uint32), want[k].view(np.uint32)
        assert np.array_equal(ug, uw), f"{what} {k}: {int((ug != uw).sum())} values differ, first at {np.argwhere(ug != uw)[0]}"


def ingest(gpu, eng, blob, n, lay, lead=0):
    """Host blob, or — `lead` > 0 — a device-resident one that starts `lead` bytes off an aligned address."""
    if not lead:
        return eng.ingest_cloud2(blob, n, lay_of(gpu, lay))
    import torch
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), np.frombuffer(blob, dtype=np.uint8)])).cuda()
    torch.cuda.synchronize()
    assert d.data_ptr() % 4 == 0
    return eng.ingest_cloud2(None, n, lay_of(gpu, lay), on_device_ptr=d.data_ptr() + lead)


@pytest.mark.parametrize("name", list(K.INGEST_CASES))
def test_decode_on_the_edges(gpu, R, name):
    """Point counts 1 ... 257 and around the scan's 262 144-point chunk, density patterns that leave waves and blocks
    empty or full, FLOAT64 intensities at every alignment and at the limits of float32, the datatypes that read as 0,
    UINT16 at an odd offset, records whose fields end on their last byte, point_step 1024, unaligned device blobs."""
    blob, lay, n, lead = K.ingest_case(name)
    eng = gpu.Engine(4.0, 4.0, 0.5)
    got = ingest(gpu, eng, blob, n, lay, lead)
    want = restate_from_cloud2(blob, n, lay)
    same_channels(got, want, name + " vs restatement")
    same_channels(got, R.from_cloud2(blob, n, lay), name + " vs oracle")
    if name == "density_none_finite":
        assert got["x"].size == 0
    elif name.startswith("density_only"):
        assert got["x"].size == 1 and got["intensity"][0] == float(name.split("_")[-1])
    elif name == "density_all_finite":
        assert got["x"].size == n
    elif name.startswith("n_"):
        assert 0.85 * n - 1 <= got["x"].size <= n
    eng.close()


def test_integrate_cloud2_over_1025_blocks(gpu, R):
    """The 262 145-point message in one call: statistics (n_input summed over 1025 block counts) and layers."""
    blob, lay, n, _ = K.ingest_case(f"n_{K.N_INTEGRATE}")
    eng, ref = pair(gpu, R, 15.0, 15.0, 0.1)
    assert (eng.rows, eng.cols) == (150, 150)
    I = np.eye(4)
    rc_e, st_e = eng.integrate_cloud2(blob, n, lay_of(gpu, lay), I, I)
    rc_r, st_r = ref.integrate_cloud2(blob, n, lay, I, I)
    assert rc_e == rc_r == 0 and st_e == st_r
    assert st_e["n_input"] == restate_from_cloud2(blob, n, lay)["x"].size < n
    assert_layers_equal(eng, ref)
    eng.close()


def test_ingest_egress_and_integrate_share_their_scratch(gpu, R):
    """`pack_counts` serves ingest, egress and the statistics of integrate_cloud2; it grows with the largest caller
    and is never cleared.  One engine runs: ingest of 300 000 points, pack of a 16 x 16 map, integrate_cloud2 of 1000
    points, pack, ingest of 5 points — each result equal to the same call on an engine that ran nothing before it."""
    case = next(c for c in K.EGRESS_CASES if c.name == "cells_256")
    big, big_lay = K.SCRATCH_BLOBS["ingest_300000"]()
    mid, mid_lay = K.SCRATCH_BLOBS["integrate_1000"]()
    few, few_lay = K.SCRATCH_BLOBS["ingest_5"]()
    I = np.eye(4)

    def fresh():
        return case.create(lambda w, h, res, fill, pos: gpu.Engine(w, h, res, fill(gpu.capi.default_config()), position=pos))[0]

    def pack(e):
        return e.pack_cloud()

    def same_pack(a, b, what):
        assert a[0] == b[0] and a[1] == b[1] and a[2].shape == b[2].shape, what
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), what

    eng = fresh()
    # 1. ingest of 300 000 points
    got = eng.ingest_cloud2(big, 300_000, lay_of(gpu, big_lay))
    same_channels(got, restate_from_cloud2(big, 300_000, big_lay), "ingest 300 000")
    e1 = gpu.Engine(4.0, 4.0, 0.5)
    same_channels(got, e1.ingest_cloud2(big, 300_000, lay_of(gpu, big_lay)), "ingest 300 000 vs fresh")
    # 2. a pack of the 16 x 16 map
    p2 = pack(eng)
    e2 = fresh()
    same_pack(p2, pack(e2), "pack after a large ingest")
    _, want = restate_pack({n: e2.layer(n) for n in e2.layers()}, e2.layers(), e2.geometry())
    assert np.array_equal(p2[2].view(np.uint32), want.view(np.uint32))
    # 3. integrate_cloud2 of 1000 points
    r3 = eng.integrate_cloud2(mid, 1000, lay_of(gpu, mid_lay), I, I)
    assert r3 == e2.integrate_cloud2(mid, 1000, lay_of(gpu, mid_lay), I, I)
    ref, _ = case.create(lambda w, h, res, fill, pos: R.RefEngine(w, h, res, fill(R.default_config()), position=pos))
    assert r3 == ref.integrate_cloud2(mid, 1000, mid_lay, I, I)
    assert r3[0] == 0 and r3[1]["n_input"] == restate_from_cloud2(mid, 1000, mid_lay)["x"].size
    # 4. a pack of the map that scan left
    p4 = pack(eng)
    same_pack(p4, pack(e2), "pack after integrate_cloud2")
    assert p4[2].shape[0] >= p2[2].shape[0] and p4[0] != p2[0]     # (the scan created the intensity layer)
    # 5. ingest of 5 points
    got = eng.ingest_cloud2(few, 5, lay_of(gpu, few_lay))
    same_channels(got, restate_from_cloud2(few, 5, few_lay), "ingest 5")
    same_channels(got, gpu.Engine(4.0, 4.0, 0.5).ingest_cloud2(few, 5, lay_of(gpu, few_lay)), "ingest 5 vs fresh")
    for e in (eng, e1, e2):
        e.close()
