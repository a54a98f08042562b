"""Inputs of the least-squares branch length tests (tests/test_ols_host.py, tests/test_gpu_ols.py): seeded, small."""
import numpy as np

from helpers.fit_inputs import balanced_slots, kind_table, table_len, trees, uniform
from phyloformer_amd import bme, fit, hostio

SIZES = (3, 4, 5, 31, 64, 65, 130)


def tables(n: int, seed: int, b: int, m: int):
    """``(preds float32 [b, P_n], slots int32 [b, m, T])``: NJ, BIONJ and caterpillar tables in turn (``fit_inputs.trees``)."""
    preds, slots, _lengths = trees(n, seed, b, m)
    return preds, slots


def four_tables(n: int, seed: int):
    """``(pred float32 [P_n], {name: slots int32 [T]})`` of one source: its NJ and BIONJ tables, a caterpillar, a balanced tree."""
    pred = np.random.default_rng(seed).uniform(0.05, 3.0, size=n * (n - 1) // 2).astype(np.float32)
    return pred, {"nj": hostio.nj_joins_host(pred[None])[0][0], "bionj": hostio.bionj_joins_host(pred[None])[0][0],
                  "caterpillar": bme.caterpillar_slots(n), "balanced": balanced_slots(n)}


def path_matrix(slots, n: int) -> np.ndarray:
    """``float64 [P_n, T]``: column k holds the pairs whose path runs over the branch of entry k (``fit.patristic_py`` of the
    k-th unit vector)."""
    width = table_len(n)
    return np.stack([fit.patristic_py(slots, np.eye(width)[k], n) for k in range(width)], axis=1)


def check_ols_files(files, stem, pred, ids, names):
    """The files of ``--ols`` of ``stem`` hold ``ols.ols_scores`` of the written tables, one line per kind of ``names``, and every
    ``.ols.nwk`` is the text of the kind's table with the OLS lengths."""
    from phyloformer_amd import ols as O
    n = len(ids)
    text = files[f"{stem}.ols.tsv"].decode()
    assert text.startswith(O.OLS_HEAD) and list(O.parse_ols_tsv(text)) == list(names)
    for row, name in zip(text.splitlines(keepends=True)[1:], names):
        slots, lengths = kind_table(name, pred)
        best, status = hostio.tree_ols_host(pred, slots)
        assert status == 0
        _tree, rows, worst_j, st = hostio.tree_fit_host(pred, np.stack([slots, slots]), np.stack([lengths, best]), patristic=False)
        assert not st.any()
        assert row == O.ols_line(name, O.ols_scores(pred, lengths, best, rows, worst_j, n))
        prefix = "" if name == "nj" else name + "."
        assert files[f"{stem}.{prefix}ols.nwk"] == hostio.newick_of_joins(slots, best, ids)
    return O.parse_ols_tsv(text)


__all__ = ["SIZES", "balanced_slots", "check_ols_files", "four_tables", "kind_table", "path_matrix", "table_len", "tables", "uniform"]
