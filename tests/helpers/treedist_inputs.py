"""The join tables the tests of the tree distances share (tests/test_treedist_host.py, tests/test_treedist_native.py,
tests/test_gpu_treedist.py): computed once per shape and never changed."""
import functools

import numpy as np

from helpers import support_inputs as si
from phyloformer_amd import bme


def random_table(n: int, rng) -> np.ndarray:
    """A valid join table of random joins (no distances behind it)."""
    out = np.zeros(2 * (n - 3) + 3, dtype=np.int32)
    alive = list(range(n))
    for t in range(n - 3):
        i, j = sorted(rng.choice(len(alive), size=2, replace=False).tolist())
        out[2 * t], out[2 * t + 1] = alive[i], alive[j]
        alive.pop(j)
    out[2 * (n - 3):] = alive
    return out


@functools.lru_cache(maxsize=None)
def random_tables(n: int, k: int, seed: int) -> np.ndarray:
    """``int32 [k][T]``: unrelated trees."""
    rng = np.random.default_rng(seed)
    out = np.stack([random_table(n, rng) for _ in range(k)])
    out.setflags(write=False)
    return out


def balanced_slots(n: int) -> np.ndarray:
    """A valid table that joins the two oldest clusters and queues the result behind the others: a balanced tree."""
    alive, slots = list(range(n)), []
    for _ in range(n - 3):
        a, b = alive[0], alive[1]
        slots += [a, b]
        alive = alive[2:] + [a]
    return np.array(slots + alive, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def mixed(n: int, k: int, seed: int = 5):
    """``(slots int32 [k][T], lengths float64 [k][T])``: NJ tables of noisy tree distances (they share many splits), the
    caterpillar, the balanced table and random tables in turn; lengths of both signs."""
    _ref, noisy = si.noisy_tables(n, 5)
    rnd = random_tables(n, k, seed + n)
    rows = []
    for i in range(k):
        rows.append((noisy[i // 4 % 5], bme.caterpillar_slots(n), balanced_slots(n), rnd[i])[i % 4] if i else noisy[0])
    slots = np.stack(rows).astype(np.int32)
    lengths = np.random.default_rng(100 * n + k).standard_normal(slots.shape)
    slots.setflags(write=False)
    lengths.setflags(write=False)
    return slots, lengths


def same(got, want):
    """Two results ``(shared, kf, wrf, status)``: integers equal, doubles bit for bit (NaN included)."""
    for g, w in zip(got, want):
        if (g is None) != (w is None):
            return False
        if g is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.shape != w.shape or g.dtype != w.dtype or g.tobytes() != w.tobytes():
            return False
    return True
