"""What the neighbour-joining tests compare against: ``nj.nj_joins`` on the float32-derived matrix, as the join table of
``pf_nj_joins``."""
import numpy as np

from phyloformer_amd import nj


def matrix_of(vec: np.ndarray, n: int) -> np.ndarray:
    """The symmetric float64 matrix of a float32 distance vector (``vec_to_phylip``'s ``dm + dm.T``)."""
    dm = np.zeros((n, n), dtype=np.float32)
    dm[np.triu_indices(n, 1)] = vec
    return (dm + dm.T).astype(np.float64)


def table_of(vec: np.ndarray, n: int):
    """``nj.nj_joins`` as the table of ``pf_nj_joins``: slots int32, lengths float64 ``[2 (n - 3) + 3]``."""
    joins, (i, j, k, li, lj, lk) = nj.nj_joins(matrix_of(vec, n))
    slots = [s for a, b, _la, _lb in joins for s in (a, b)] + [i, j, k]
    lengths = [x for _a, _b, la, lb in joins for x in (la, lb)] + [li, lj, lk]
    return np.array(slots, dtype=np.int32), np.array(lengths, dtype=np.float64)


def assert_table(slots, lengths, vec, n):
    """Slots equal, lengths equal as uint64."""
    want_s, want_l = table_of(vec, n)
    assert np.array_equal(slots, want_s)
    assert np.array_equal(np.ascontiguousarray(lengths).view(np.uint64), want_l.view(np.uint64))


def tie_cases(n: int = 23) -> np.ndarray:
    """float32 [3][P_n]: all-equal distances (every Q ties at every join), duplicated sequences (zero distances and the
    ties among them), and all-equal with negative zeros (``x + 0.0f``: they enter as +0)."""
    p = n * (n - 1) // 2
    equal = np.full(p, 0.75, dtype=np.float32)
    iu = np.triu_indices(n, 1)
    full = np.zeros((n, n), dtype=np.float32)
    full[iu] = np.random.default_rng(5).uniform(0.01, 3.0, size=p).astype(np.float32)
    full = full + full.T
    for a, b in ((2, 7), (7, 11), (15, 16)):         # row b becomes a copy of row a
        full[b, :] = full[a, :]
        full[:, b] = full[:, a]
        full[a, b] = full[b, a] = 0.0
    full[2, 11] = full[11, 2] = 0.0
    np.fill_diagonal(full, 0.0)
    neg0 = equal.copy()
    neg0[::3] = -0.0
    return np.stack([equal, full[iu], neg0])
