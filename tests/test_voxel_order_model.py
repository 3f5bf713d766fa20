"""The restatement of libstdc++'s std::sort that option voxel_any_order = 1 reproduces on the device
(scripts/introsort_model.py, fdm_introsort.hpp), checked on the CPU against the oracle's std::sort."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import introsort_model as M  # noqa: E402

F32 = np.float32


def oracle_pick(R, keys, stable=False):
    x = np.asarray(keys, dtype=F32) + F32(0.5)
    zero = np.zeros(len(keys), dtype=F32)
    return list(R.voxel_any(x, zero, zero, 1.0, stable=stable))


def model_pick(keys):
    order = M.std_sort(keys)
    return M.voxel_pick([keys[i] for i in order], order)


def test_closed_form_partition_matches_the_loop():
    rng = np.random.default_rng(11)
    for _ in range(3000):
        m = int(rng.integers(17, 120))
        k = [int(v) for v in rng.integers(0, int(rng.choice([2, 4, 40])), m)]
        mp = M.median_to_first(k, 1, m // 2, m - 1)
        k[0], k[mp] = k[mp], k[0]
        assert M.partition_closed(k, 0, m) == M.partition_literal(k, 0, m)


@pytest.mark.parametrize("shape", ["random", "sorted", "reversed", "organ_pipe", "alternating", "all_equal"])
@pytest.mark.parametrize("n", [1, 2, 16, 17, 31, 33, 1000, 2500])
def test_model_matches_std_sort(R, n, shape):
    rng = np.random.default_rng(n * 7 + len(shape))
    keys = [int(v) for v in rng.integers(0, max(2, n // 6), n)]
    if shape == "sorted":
        keys.sort()
    elif shape == "reversed":
        keys.sort(reverse=True)
    elif shape == "organ_pipe":
        keys = [min(i, n - 1 - i) // 3 for i in range(n)]
    elif shape == "alternating":
        keys = [i % 2 for i in range(n)]
    elif shape == "all_equal":
        keys = [3] * n
    assert model_pick(keys) == oracle_pick(R, keys)


@pytest.mark.parametrize("n", [200, 2000, 5000])
def test_median_of_3_killer_reaches_the_heap_fallback(R, n):
    keys = M.median3_killer(n)
    rep = {}
    M.std_sort(keys, rep)
    assert any(ties for _, _, ties in rep["heap_ranges"]), rep["heap_ranges"]
    assert model_pick(keys) == oracle_pick(R, keys)
    assert oracle_pick(R, keys) != oracle_pick(R, keys, stable=True)
