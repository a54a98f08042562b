"""The join tables the tests of the split supports share (tests/test_supports_host.py, tests/test_gpu_supports.py):
computed once per shape and never changed."""
import functools

import numpy as np

from helpers import bme_check as bc
from phyloformer_amd import bme


def nj_table(vec: np.ndarray, n: int) -> np.ndarray:
    return bme.nj_start(bme.matrix_of_preds(vec, n))


@functools.lru_cache(maxsize=None)
def noisy_tables(n: int, r: int, noise: float = 0.2):
    """``(ref int32 [T], reps int32 [r][T])``: the NJ table of ``random_tree_distances(n, 3)`` and those of the same
    distances times ``1 + noise * gaussian``."""
    base = bc.random_tree_distances(n, 3)
    g = np.random.default_rng(1000 * n + r).standard_normal((r,) + base.shape)
    reps = np.stack([nj_table((base * (1 + noise * g[k])).astype(np.float32), n) for k in range(r)])
    ref = nj_table(base, n)
    ref.setflags(write=False)
    reps.setflags(write=False)
    return ref, reps


@functools.lru_cache(maxsize=None)
def unrelated_tables(n: int, r: int):
    """``int32 [r][T]``: the NJ tables of ``uniform_preds(n, 11, r)``."""
    reps = np.stack([nj_table(v, n) for v in bc.uniform_preds(n, 11, r)])
    reps.setflags(write=False)
    return reps


@functools.lru_cache(maxsize=None)
def sources(n: int, r: int):
    """Two sources ``(ref int32 [2][T], reps int32 [2][r][T], flag bool [2][r])`` that reach every branch of the
    definition: source 0 has noisy replicates, the last of them (``r > 1``) the reference itself; source 1 has unrelated
    replicates, the last of them (``r > 1``) passed with its flag set and a table of zeros, which must not be read."""
    ref, noisy = noisy_tables(n, r)
    reps = np.stack([noisy, unrelated_tables(n, r)])
    flag = np.zeros((2, r), dtype=bool)
    if r > 1:
        reps[0, r - 1] = ref
        reps[1, r - 1] = 0
        flag[1, r - 1] = True
    out = (np.stack([ref, ref]), reps, flag)
    for a in out:
        a.setflags(write=False)
    return out
