"""Inputs of the tree-fit tests (tests/test_fit_host.py, tests/test_gpu_fit.py): seeded, small."""
import numpy as np

from phyloformer_amd import bme, hostio


def pairs_of(n: int) -> int:
    return n * (n - 1) // 2


def table_len(n: int) -> int:
    return 2 * (n - 3) + 3


def uniform(n: int, seed: int, b: int = 1) -> np.ndarray:
    """``float32 [b, P_n]`` in (0.01, 3)."""
    return np.random.default_rng(seed).uniform(0.01, 3.0, size=(b, pairs_of(n))).astype(np.float32)


def balanced_slots(n: int) -> np.ndarray:
    """The join table ``int32 [T]`` of a balanced tree: rounds of joins of neighbouring live slots, so a leaf is about
    ``log2 n`` nodes below the last one."""
    live, table = list(range(n)), []
    while len(live) > 3:
        nxt, k, count = [], 0, len(live)
        while k < len(live):
            if k + 1 < len(live) and count > 3:
                table += [live[k], live[k + 1]]
                nxt.append(live[k])
                k += 2
                count -= 1
            else:
                nxt.append(live[k])
                k += 1
        live = nxt
    return np.array(table + live, dtype=np.int32)


def trees(n: int, seed: int, b: int, m: int):
    """``(preds float32 [b, P_n], slots int32 [b, m, T], lengths float64 [b, m, T])``: tree 0 of a source is its NJ table (with
    the negative lengths NJ gives random distances), tree 1 its BIONJ table, tree 2 a caterpillar (``bme.caterpillar_slots``)
    with random lengths, a tenth of them negative."""
    rng = np.random.default_rng(seed + 17)
    preds = uniform(n, seed, b)
    made = [hostio.nj_joins_host(preds)[:2], hostio.bionj_joins_host(preds)[:2],
            (np.broadcast_to(bme.caterpillar_slots(n), (b, table_len(n))), rng.uniform(-0.1, 0.9, size=(b, table_len(n))))]
    slots = np.stack([np.asarray(made[k % 3][0], dtype=np.int32) for k in range(m)], axis=1)
    lengths = np.stack([np.asarray(made[k % 3][1], dtype=np.float64) for k in range(m)], axis=1)
    return preds, np.ascontiguousarray(slots), np.ascontiguousarray(lengths)


def same(a, b) -> bool:
    """Equal arrays, float64 by their bits."""
    def bits(x):
        x = np.ascontiguousarray(x)
        return x.view(np.uint64) if x.dtype == np.float64 else x
    return all((x is None and y is None) or (np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).shape == np.asarray(y).shape
                                              and np.array_equal(bits(np.asarray(x)), bits(np.asarray(y)))) for x, y in zip(a, b))


def kind_table(name: str, pred: np.ndarray):
    """``(slots, lengths)`` of the tree of kind ``name`` (``treekinds.KINDS``) of one source, on the host."""
    from phyloformer_amd import treekinds
    kind = next(k for k in treekinds.KINDS if k.name == name)
    made = treekinds.join_refine(treekinds.NativeHost(), kind.start, [kind.search] if kind.search else [], pred[None])
    slots, lengths, _steps, bad = made[kind.search]
    assert not bad[0]
    return slots[0], lengths[0]


def check_fit_files(files, stem, pred, ids, names):
    """The files of ``--fit`` of ``stem`` hold ``fit.fit_scores`` of the written tables, one line per kind of ``names``, and
    every written tree is the text of its table."""
    from phyloformer_amd import fit as F
    from phyloformer_amd.phylip import vec_to_phylip
    n = len(ids)
    text = files[f"{stem}.fit.tsv"].decode()
    assert text.startswith(F.FIT_HEAD) and list(F.parse_fit_tsv(text)) == list(names)
    for row, name in zip(text.splitlines(keepends=True)[1:], names):
        slots, lengths = kind_table(name, pred)
        assert files[f"{stem}.{name}.nwk"] == hostio.newick_of_joins(slots, lengths, ids)
        tree, rows, worst_j, status = hostio.tree_fit_host(pred, slots, lengths)
        assert status == 0
        s = F.fit_scores(pred, rows, worst_j, n)
        assert row == F.fit_line(name, s)
        prefix = "" if name == "nj" else name + "."
        assert files[f"{stem}.{prefix}fit.taxa.tsv"].decode() == F.taxa_tsv(ids, s)
        assert files[f"{stem}.{prefix}patristic.phy"].decode() == vec_to_phylip(tree.astype(np.float32), ids)[1]
    return F.parse_fit_tsv(text)
