"""Every kernel the stencil stages choose between (fdm_engine_post.inl), reached through the plain calls with parameters
the reference accepts, against the oracle: the engine says which kernel it launched (Engine.debug_last_post_kernel) and
every layer matches bit for bit.  The cases, their fields and the name each must run are tests/post_cases.py;
tests/test_post_cases.py proves on the CPU that the cases do what they are meant to and leave no launch site out.

Tolerance: none.  Inpainting, the median and the fusion repeat the reference's float operations in its order; feature
extraction does once both sides round atan2 / cos / sin / acos correctly (the device does; the oracle's trig_mode 1).
"""
import numpy as np
import pytest

import post_cases as PC
from helpers import assert_arrays_close, pair

pytestmark = pytest.mark.gpu


def exact(eng, ref):
    assert sorted(eng.layers()) == sorted(ref.layers())
    for n in ref.layers():
        assert_arrays_close(eng.layer(n), ref.layer(n), n, 0.0, 0.0)


def rolled_pair(gpu, R, map_name):
    width, height, rows, cols, shift = PC.MAPS[map_name]
    eng, ref = pair(gpu, R, width, height, PC.RES)
    for o in (eng, ref):
        o.move(*shift)  # the circular buffer's seam crosses the map
    assert (eng.rows, eng.cols) == (ref.rows, ref.cols) == (rows, cols)
    return eng, ref


@pytest.fixture()
def rounded_trig(R):
    R.set_trig_mode(1)
    yield
    R.set_trig_mode(0)


@pytest.mark.parametrize("case", PC.CASES, ids=[c.id for c in PC.CASES])
def test_case_runs_its_kernel_and_matches_the_oracle(gpu, R, rounded_trig, case):
    eng, ref = rolled_pair(gpu, R, case.map)
    # twice from the same input (the second call finds its region table, and a pooled kernel its pool, on the device),
    # then with a changed radius / size: another table, another pool
    for params, kernel in ((case.params, case.kernel), (case.params, case.kernel),
                           (case.again, PC.kernel_of(case.stage, case.again))):
        for o in (eng, ref):
            PC.set_layers(o, case)
            PC.apply(o, case.stage, params)
        assert eng.debug_last_post_kernel() == kernel, (case.id, params)
        exact(eng, ref)
    for n in PC.OUTPUTS[case.stage]:
        assert eng.exists(n) or (case.stage == "inpaint" and n == "elevation_inpainted")


def test_calls_that_launch_nothing_record_the_empty_name(gpu, R):
    eng, ref = rolled_pair(gpu, R, "small")
    case = next(c for c in PC.CASES if c.id == "median-17")
    PC.set_layers(eng, case)
    PC.apply(eng, case.stage, case.params)
    assert eng.debug_last_post_kernel() == "k_median_sel"
    eng.apply_spatial_smoothing("nonexistent_layer", 17, 5)          # a missing layer
    assert eng.debug_last_post_kernel() == ""
    PC.apply(eng, case.stage, case.params)
    eng.apply_inpainting(0, 2)                                        # no pass
    assert eng.debug_last_post_kernel() == ""
    up, lo = PC.bound_field((eng.rows, eng.cols), 5)
    for o in (eng, ref):
        o.set_layer("upper_bound", up)
        o.set_layer("lower_bound", lo)
        o.apply_uncertainty_fusion(True, PC.cells(3.2), 0.1, 0.01, 0.99, 3)
    assert eng.debug_last_post_kernel() == "k_fusion_wave"
    for o in (eng, ref):
        o.apply_uncertainty_fusion(False, PC.cells(3.2), 0.1, 0.01, 0.99, 3)   # disabled
    assert eng.debug_last_post_kernel() == ""
    for n in ("upper_bound", "lower_bound"):
        assert_arrays_close(eng.layer(n), ref.layer(n), n, 0.0, 0.0)
    bare, _ = rolled_pair(gpu, R, "strip")
    assert bare.debug_last_post_kernel() == ""                                  # no stage yet
    bare.apply_uncertainty_fusion(True, PC.cells(3.2), 0.1, 0.01, 0.99, 3)      # without bound layers: nothing to launch
    assert bare.debug_last_post_kernel() == ("k_fusion_wave" if bare.exists("upper_bound") else "")
