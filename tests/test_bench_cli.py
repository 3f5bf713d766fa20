"""bench.py's command line (no GPU): what a step is for each workload, and the defaults the driver relies on
(`python bench.py` alone must pick N = 1 and a K / W that finish within minutes)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv):
    import bench
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_defaults():
    a = parse([])
    assert (a.gpus, a.workload, a.steps, a.warmup) == (1, "c2", 625, 64)  # 625 steps x 16 scans = 10 000 scans
    assert a.scans_per_step == 0  # = per workload: 16 for the small-scan workloads, 1 for the large-scan ones


def test_driver_arguments_are_taken_literally():
    a = parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert (a.gpus, a.steps, a.warmup) == (1, 20, 5)


def test_full_is_off_unless_asked_for():
    """A plain run measures the headline alone; the legs beside it ride behind --full, which changes no step count."""
    assert parse(["--gpus", "1", "--steps", "20", "--warmup", "5"]).full is False
    a = parse(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert a.full is True and (a.gpus, a.steps, a.warmup) == (1, 20, 5)


def test_large_scan_workloads_step_per_scan():
    a = parse(["--workload", "c4"])
    assert (a.steps, a.warmup) == (10000, 1000)
    b = parse(["--workload", "c2", "--scans-per-step", "1"])
    assert (b.steps, b.warmup) == (10000, 1000)


def test_gpus_follows_the_launcher_when_it_is_not_given(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "4")
    assert parse([]).gpus == 4
    assert parse(["--gpus", "2"]).gpus == 2  # (main() then refuses: the launcher started another number of ranks)
    monkeypatch.delenv("WORLD_SIZE")
    assert parse([]).gpus == 1


def test_gpus_n_without_a_launcher_spawns_n_ranks_before_any_gpu_call(monkeypatch):
    """`python bench.py --gpus 8` the way the driver runs `--gpus 1`: no WORLD_SIZE in the environment, so bench.py
    itself starts the ranks through torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1) and leaves
    with the launcher's exit code — before it imports torch, let alone touches the GPU."""
    import bench
    calls = {}

    def fake_call(cmd, env=None):
        calls["cmd"], calls["env"] = cmd, env
        return 7

    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "5"])
    sys.modules.pop("torch", None) if "torch" in sys.modules and False else None
    import pytest
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert ex.value.code == 7  # a failing rank -> non-zero exit
    cmd = calls["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"] and cmd[-7].endswith("bench.py")
    assert calls["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_world_size_must_match_gpus(monkeypatch):
    import bench
    import pytest
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        bench.main()


def test_watchdog_hands_a_stall_to_its_callback():
    """tiling.Watchdog: a rank that makes no progress leaves — through `on_stall` when one is given (bench.py's riding
    global-map leg prints the replicas' line there and leaves with code 0), else with code 3."""
    code = ("import os, sys, time; sys.path.insert(0, %r); from fastdem_amd.tiling import Watchdog;"
            "w = Watchdog(0.3, what='t', on_stall=(lambda m: (print('STALL', m), sys.stdout.flush(), os._exit(0))) if sys.argv[1] == 'cb' else None);"
            "time.sleep(5); print('not reached')") % ROOT
    r = subprocess.run([sys.executable, "-c", code, "cb"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "STALL" in r.stdout and "not reached" not in r.stdout, (r.returncode, r.stdout, r.stderr)
    r = subprocess.run([sys.executable, "-c", code, "plain"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "no progress" in r.stderr, (r.returncode, r.stdout, r.stderr)


def test_routed_global_map_defaults_are_the_steps_it_runs():
    """c5 (routed: one global map over the ranks) times exactly --steps routed steps; its default is 200 of them."""
    a = parse(["--workload", "c5"])
    assert (a.steps, a.warmup) == (200, 400)
    assert (parse(["--workload", "c5", "--steps", "1000"]).steps) == 1000
    b = parse(["--workload", "c5", "--routed", "0"])  # (one plain engine on the whole map: a scan per step)
    assert (b.steps, b.warmup) == (10000, 1000)


class _FakeEngine:
    """What bench.dump_outputs reads of an Engine, over numpy arrays (no GPU); unobserved cells are NaN, a few +-inf."""

    def __init__(self, rows, cols, names):
        import numpy as np
        from fastdem_amd import capi
        self.s_rows, self.s_cols = rows, cols
        rng = np.random.default_rng(1)
        self.data = {}
        for n in names:
            a = rng.standard_normal((rows, cols)).astype(np.float32)
            a[rng.random((rows, cols)) < 0.3] = np.nan
            a[0, 0], a[0, 1] = np.inf, -np.inf
            self.data[n] = np.asfortranarray(a)
        self.g = capi.FdmGeometry(length_x=rows * 0.1, length_y=cols * 0.1, resolution=0.1, position_x=1.5,
                                  position_y=-2.0, rows=rows, cols=cols, start_row=3, start_col=4)
        self.synced = False

    def sync(self):
        self.synced = True

    def layers(self):
        return list(self.data) + ["_internal"]

    def layer(self, name):
        return self.data[name]

    def geometry(self):
        return self.g

    def last_stats(self):
        return 0, {"n_input": 30000, "n_after_filter": 29000, "n_in_map": 28000, "n_cells_touched": 900,
                   "shift_rows": -1, "shift_cols": 2}


def _decoded(out, name):
    """A dumped layer with its non-finite cells put back from `_nonfinite_<name>`; every stored value must be finite."""
    import numpy as np
    v, code = np.load(out / f"{name}.npy"), np.load(out / f"_nonfinite_{name}.npy")
    assert v.dtype == code.dtype == np.float32 and v.shape == code.shape
    assert np.isfinite(v).all() and np.isin(code, (0, 1, 2, 3)).all() and not v[code != 0].any()
    return np.select([code == 1, code == 2, code == 3], [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)], v)


def test_dump_outputs_writes_every_layer_geometry_and_stats(tmp_path):
    import numpy as np
    import bench
    eng = _FakeEngine(30, 20, ["elevation", "variance", "color"])
    out = tmp_path / "out"
    bench.dump_outputs(eng, str(out))
    files = sorted(p.name for p in out.iterdir())
    assert files == sorted(["_geometry.npy", "_scan_stats.npy"] +
                           [f"{p}{n}.npy" for n in ("color", "elevation", "variance") for p in ("", "_nonfinite_")])
    assert eng.synced
    assert all(np.isfinite(np.load(out / f)).all() for f in files)
    for n in ("elevation", "variance", "color"):
        a = _decoded(out, n)
        assert a.shape == (30, 20)
        assert np.array_equal(a.view(np.uint32), eng.data[n].view(np.uint32))  # (NaN payloads: the engine's canonical NaN)
    geo = np.load(out / "_geometry.npy")
    assert geo.dtype == np.float64 and geo.tolist() == [3.0, 2.0, 0.1, 1.5, -2.0, 30, 20, 3, 4]
    st = np.load(out / "_scan_stats.npy")
    assert st.dtype == np.float64 and st.tolist() == [30000, 29000, 28000, 900, -1, 2]


def test_dump_outputs_samples_a_large_map_within_the_budget(tmp_path):
    """A map larger than the budget: the same seeded cells of every layer, the same cells from run to run."""
    import numpy as np
    import bench
    eng = _FakeEngine(600, 500, ["elevation", "variance"])
    budget = (1 << 20) + 400_000
    for d in ("a", "b"):
        bench.dump_outputs(eng, str(tmp_path / d), budget=budget)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= budget
    assert all(np.isfinite(np.load(tmp_path / "a" / f)).all() for f in files)
    idx = np.load(tmp_path / "a" / "_sample_cells.npy")
    assert idx.dtype == np.float64 and 0 < idx.size < 600 * 500 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "_sample_cells.npy"))
    flat = eng.data["elevation"].ravel(order="F")
    e = _decoded(tmp_path / "a", "elevation")
    assert np.array_equal(e, flat[idx.astype(np.int64)], equal_nan=True)
    for f in files:
        assert np.load(tmp_path / "a" / f).tobytes() == np.load(tmp_path / "b" / f).tobytes(), f
