"""What the BIONJ tests compare against: ``bionj.bionj_joins`` on the float32-derived matrix, as the join table of
``pf_bionj_joins``; and the constructed inputs the tests share."""
import numpy as np

from helpers.nj_table import matrix_of
from phyloformer_amd import bionj


def table_of(vec: np.ndarray, n: int):
    """``bionj.bionj_joins`` as the table of ``pf_bionj_joins``: slots int32, lengths float64 ``[2 (n - 3) + 3]``."""
    return bionj.bionj_table(matrix_of(vec, n))


def assert_table(slots, lengths, vec, n):
    """Slots equal, lengths equal as uint64."""
    want_s, want_l = table_of(vec, n)
    assert np.array_equal(slots, want_s)
    assert np.array_equal(np.ascontiguousarray(lengths).view(np.uint64), want_l.view(np.uint64))


def assert_tables_equal(got, want):
    """Two ``(slots, lengths, ...)`` results: slots equal, lengths equal as uint64."""
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))


def uniform(n: int, seed: int, b: int = 1) -> np.ndarray:
    """float32 [b][P_n], uniform in (0.01, 3)."""
    return np.random.default_rng(seed).uniform(0.01, 3.0, size=(b, n * (n - 1) // 2)).astype(np.float32)


def duplicated_rows(n: int, seed: int, copies=((1, 4), (4, 6), (2, 3))) -> np.ndarray:
    """float32 [P_n]: random distances in which row ``b`` is a copy of row ``a`` and ``d_ab = 0`` for every ``(a, b)`` of
    ``copies`` - identical sequences: rounding-level ties of ``q`` (the window) and ``v_ab = 0`` (``lambda = 1/2``)."""
    iu = np.triu_indices(n, 1)
    full = np.zeros((n, n), dtype=np.float32)
    full[iu] = uniform(n, seed)[0]
    full = full + full.T
    for a, b in copies:
        full[b, :] = full[a, :]
        full[:, b] = full[:, a]
        full[a, b] = full[b, a] = 0.0
    for a, b in copies:                                # chains of copies: every pair inside a group is at zero
        for c, e in copies:
            if b == c:
                full[a, e] = full[e, a] = 0.0
    np.fill_diagonal(full, 0.0)
    return full[iu]
