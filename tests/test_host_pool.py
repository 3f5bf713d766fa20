"""fdm_host_alloc / fdm_host_free (include/fdm_engine.h): pooled pinned memory for input clouds.
Without a GPU the blocks are ordinary memory (the engine would copy them); on a GPU box they are
pinned, pooled, and read in place by the synchronous host entry points too."""
import numpy as np
import pytest

F32 = np.float32


def test_blocks_without_a_gpu_are_plain_memory():
    import torch
    import fastdem_amd
    if torch.cuda.is_available():
        pytest.skip("pageable fallback is only taken without a GPU")
    h = fastdem_amd.host_array(np.arange(1000, dtype=F32))
    assert not h.pinned
    assert np.array_equal(h.array, np.arange(1000, dtype=F32))
    lib = fastdem_amd.capi.load()
    lib.fdm_host_free(None)
    lib.fdm_host_trim()
    del h


def test_zero_length_block():
    import fastdem_amd
    h = fastdem_amd.HostArray(0)
    assert h.array.size == 0


@pytest.mark.gpu
def test_pool_reuses_pinned_blocks(gpu):
    lib = gpu.capi.load()
    a = lib.fdm_host_alloc(300000)
    assert lib.fdm_host_is_pinned(a) == 1
    lib.fdm_host_free(a)
    b = lib.fdm_host_alloc(270000)  # same 512 KiB class
    assert a == b
    lib.fdm_host_free(b)
    lib.fdm_host_trim()
    big = lib.fdm_host_alloc((1 << 30) + 4096)  # above the largest class: not pooled
    assert big and lib.fdm_host_is_pinned(big) == 1
    lib.fdm_host_free(big)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["integrate", "update"])
def test_synchronous_entry_points_read_pinned_arrays_in_place(gpu, R, entry):
    """fdm_engine_integrate / fdm_engine_update on pooled pinned arrays (no copy commands) against the
    oracle, stats included; odd sizes and a z-variance channel exercise the write-through of the
    channels only the update kernel consumes."""
    from helpers import assert_layers_equal, pair, same_geometry
    wl = gpu.synth.vlp16(n_scans=3)
    eng, ref = pair(gpu, R, wl.width, wl.height, wl.resolution, wl.apply_to)
    rng = np.random.default_rng(3)
    for k in range(3):
        s = wl.scan(k)
        n = s["x"].size - 7 * k - 1
        ch = {c: gpu.host_array(s[c][:n]) for c in ("x", "y", "z", "intensity")}
        assert all(h.pinned for h in ch.values())
        if entry == "integrate":
            out_e = eng.integrate(ch["x"].array, ch["y"].array, ch["z"].array, wl.T_base_sensor, wl.pose(k),
                                  intensity=ch["intensity"].array)
            out_r = ref.integrate(s["x"][:n], s["y"][:n], s["z"][:n], wl.T_base_sensor, wl.pose(k),
                                  intensity=s["intensity"][:n])
        else:
            var = gpu.host_array(rng.uniform(1e-4, 5e-3, n).astype(F32))
            out_e = eng.update(ch["x"].array, ch["y"].array, ch["z"].array, (0.1 * k, -0.2 * k), z_var=var.array,
                               intensity=ch["intensity"].array)
            out_r = ref.update(s["x"][:n], s["y"][:n], s["z"][:n], (0.1 * k, -0.2 * k), z_var=var.array.copy(),
                               intensity=s["intensity"][:n])
        assert out_e == out_r
    assert_layers_equal(eng, ref)
    assert same_geometry(eng.geometry(), ref.geometry())


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["integrate", "integrate_async", "integrate_host_batch"])
def test_a_scan_is_read_in_place_only_if_every_channel_present_is_pinned(gpu, R, entry):
    """One rule decides for the three host entry points whether a scan is read in place: every channel it has is pinned
    (and the scan within the zero_copy bound).  Two scans with intensity and colour into a 64 x 64-cell map, 1 000 and
    1 025 points (one past a 1 024-point block, so the channel offsets inside a staging slot matter), each from pageable
    arrays (against the oracle), from pinned arrays, from x / z / rgb pinned with y / intensity pageable, and from pinned
    arrays with zero_copy = 0: every layer bit for bit what the pageable run left."""
    import ctypes as C
    from helpers import assert_layers_bit_identical, assert_layers_equal, pair, same_geometry
    wl = gpu.synth.vlp16(n_scans=2)
    rng = np.random.default_rng(11)
    channels = ("x", "y", "z", "intensity", "rgb")
    scans = []
    for k, n in enumerate((1000, 1025)):
        s = wl.scan(k)
        pick = np.arange(n) * (s["x"].size // n)  # spread over the whole sweep
        d = {c: np.ascontiguousarray(s[c][pick]) for c in ("x", "y", "z", "intensity")}
        d["rgb"] = rng.integers(0, 1 << 24, n, dtype=np.uint32)
        scans.append(d)
    keep = []  # the arrays stay untouched until the engine that read them has been waited for

    def arrays(s, pinned):
        out = {}
        for c in channels:
            if c in pinned:
                h = gpu.host_array(s[c], s[c].dtype)
                assert h.pinned
                keep.append(h)
                out[c] = h.array
            else:
                out[c] = s[c].copy()
                keep.append(out[c])
        return out

    def mat16(m):
        return (C.c_double * 16)(*np.ascontiguousarray(np.asarray(m, dtype=np.float64).T).reshape(16))

    def run(pinned, zero_copy=None, with_oracle=False):
        eng, ref = pair(gpu, R, 8.0, 8.0, 0.125, wl.apply_to)
        assert (eng.s_rows, eng.s_cols) == (64, 64)
        eng.enable_cell_ids(False)
        if zero_copy is not None:
            eng.set_option("zero_copy", zero_copy)
        a = [arrays(s, pinned) for s in scans]
        outs = []
        if entry == "integrate_host_batch":
            arr = (gpu.capi.FdmDeviceScan * len(a))()
            for k, ch in enumerate(a):
                d = arr[k]
                d.n = int(ch["x"].size)
                for c in channels:
                    setattr(d, c, ch[c].ctypes.data)
                d.sigma_z2 = None
                d.T_base_sensor, d.T_world_base = mat16(wl.T_base_sensor), mat16(wl.pose(k))
            outs.append(eng.integrate_host_batch(arr))
        else:
            for k, ch in enumerate(a):
                args = (ch["x"], ch["y"], ch["z"], wl.T_base_sensor, wl.pose(k))
                if entry == "integrate":
                    outs.append(eng.integrate(*args, intensity=ch["intensity"], rgb=ch["rgb"]))
                else:
                    eng.integrate_async(*args, intensity=ch["intensity"], rgb=ch["rgb"])
            if entry == "integrate_async":
                eng.sync()
                outs.append(eng.last_stats())
        if with_oracle:
            outs_r = [ref.integrate(s["x"], s["y"], s["z"], wl.T_base_sensor, wl.pose(k), intensity=s["intensity"],
                                    rgb=s["rgb"]) for k, s in enumerate(scans)]
            assert outs == outs_r[-len(outs):]
            assert_layers_equal(eng, ref)
            assert same_geometry(eng.geometry(), ref.geometry())
        return eng

    pageable = run((), with_oracle=True)
    for pinned, zero_copy in ((channels, None), (("x", "z", "rgb"), None), (channels, 0), (("x", "z", "rgb"), 0)):
        eng = run(pinned, zero_copy)
        assert_layers_bit_identical(eng, pageable)
        assert same_geometry(eng.geometry(), pageable.geometry())
