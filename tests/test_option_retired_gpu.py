"""The seventeen retired engine options (tests/test_option_table.py, RETIRED) are unknown to fdm_engine_set_option, and an
engine that was asked for them goes on working."""
import numpy as np
import pytest

from test_option_table import RETIRED

pytestmark = pytest.mark.gpu


def test_retired_options_are_refused(gpu):
    lib = gpu.capi.load()
    eng = gpu.Engine(0.8, 0.8, 0.1)
    assert (eng.rows, eng.cols) == (8, 8)
    assert len(RETIRED) == 17
    for name in RETIRED:
        for value in (0, 1):
            rc = lib.fdm_engine_set_option(eng._h, name.encode(), value)
            assert rc == gpu.capi.FDM_ERR_INVALID, (name, value, rc)
            assert lib.fdm_last_error().decode() == "unknown option " + name
    eng.set_option("overlap", 1)      # (a row of the table still is an option)
    rng = np.random.default_rng(5)
    x, y = (rng.uniform(-0.39, 0.39, 200).astype(np.float32) for _ in range(2))
    z = rng.uniform(-0.2, 0.2, 200).astype(np.float32)
    rc, st = eng.integrate(x, y, z, np.eye(4), np.eye(4))
    assert rc == 0, (rc, st)
    elevation = eng.layer("elevation")
    assert elevation.shape == (8, 8) and np.isfinite(elevation).sum() > 32
