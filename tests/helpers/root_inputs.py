"""Inputs of the tree rooting tests (tests/test_root_host.py, tests/test_gpu_root.py): seeded, small."""
import numpy as np

from helpers.fit_inputs import balanced_slots, kind_table, same, table_len, uniform
from phyloformer_amd import bme, hostio

SIZES = (3, 4, 5, 31, 64, 65, 130)
# k_root_score walks places in groups of 256 and partners in chunks of 256: the two sizes around that edge as well
GPU_SIZES = SIZES + (256, 257)
CLOCK_SIZES = (4, 5, 9, 17, 33, 65, 130)


def tables(n: int, seed: int, b: int, m: int):
    """``(slots int32 [b, m, T], lengths float64 [b, m, T])``: NJ, BIONJ, caterpillar and balanced tables in turn, source ``k`` starting
    with kind ``k``; NJ and BIONJ lengths of random distances (some negative), random lengths in (-0.1, 0.9) on the other two."""
    rng = np.random.default_rng(seed + 17)
    preds = uniform(n, seed, b)
    width = table_len(n)
    made = [hostio.nj_joins_host(preds)[:2], hostio.bionj_joins_host(preds)[:2],
            (np.broadcast_to(bme.caterpillar_slots(n), (b, width)), rng.uniform(-0.1, 0.9, size=(b, width))),
            (np.broadcast_to(balanced_slots(n), (b, width)), rng.uniform(-0.1, 0.9, size=(b, width)))]
    slots, lengths = np.zeros((b, m, width), dtype=np.int32), np.zeros((b, m, width), dtype=np.float64)
    for k in range(b):
        for r in range(m):
            slots[k, r], lengths[k, r] = made[(k + r) % 4][0][k], made[(k + r) % 4][1][k]
    return slots, lengths


def clock_tree(n: int, seed: int):
    """A coalescent of ``n`` leaves with node heights in multiples of 2^-10: ``(dm float64 [n, n], left, right, heights)`` - the
    additive distances ``2 x height of the common ancestor``, the leaf sets of the root's two children and their heights."""
    rng = np.random.default_rng(seed)
    groups = [([x], 0.0) for x in range(n)]
    dm = np.zeros((n, n), dtype=np.float64)
    height = 0.0
    while len(groups) > 1:
        height += int(rng.integers(8, 64)) / 1024.0
        i, j = sorted(rng.choice(len(groups), size=2, replace=False).tolist())
        (a, ha), (b, hb) = groups[i], groups[j]
        for x in a:
            for y in b:
                dm[x, y] = dm[y, x] = 2.0 * height
        last = (a, b, ha, hb)
        groups[i] = (a + b, height)
        groups.pop(j)
    return dm, sorted(last[0]), sorted(last[1]), (last[2], last[3], height)


def pairs_of_matrix(dm: np.ndarray) -> np.ndarray:
    n = len(dm)
    return np.array([dm[i, j] for i in range(n) for j in range(i + 1, n)])


__all__ = ["CLOCK_SIZES", "GPU_SIZES", "SIZES", "balanced_slots", "clock_tree", "kind_table", "pairs_of_matrix", "same", "table_len", "tables",
           "uniform"]
