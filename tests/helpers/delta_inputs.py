"""Inputs of the delta-score tests (tests/test_delta_host.py, tests/test_gpu_delta.py): seeded, small."""
from itertools import combinations
from math import comb

import numpy as np
import pytest

from phyloformer_amd import delta as D


def pairs_of(n: int) -> int:
    return n * (n - 1) // 2


def uniform(n: int, seed: int, b: int = 1) -> np.ndarray:
    """``float32 [b, P_n]`` in (0.01, 3)."""
    return np.random.default_rng(seed).uniform(0.01, 3.0, size=(b, pairs_of(n))).astype(np.float32)


def small_integers(n: int, seed: int, b: int = 1, top: int = 4) -> np.ndarray:
    """``float32 [b, P_n]`` of integers in [0, top): many equal sums, zero denominators and halves."""
    return np.random.default_rng(seed).integers(0, top, size=(b, pairs_of(n))).astype(np.float32)


def mixed(n: int, seed: int, b: int) -> np.ndarray:
    """``b`` sources: random ones; from two on the last is of small integers; from three on the middle one holds a NaN (an
    infinity for an odd seed)."""
    p = uniform(n, seed, b)
    if b >= 2:
        p[-1] = small_integers(n, seed + 1)[0]
    if b >= 3:
        p[b // 2, (seed * 7) % pairs_of(n)] = np.inf if seed % 2 else np.nan
    return p


def tree_distances(n: int, seed: int) -> np.ndarray:
    """Patristic distances ``float32 [P_n]`` of a random binary tree with INTEGER branch lengths in [1, 9] (exact in
    float32, so every quartet satisfies the four-point condition exactly)."""
    rng = np.random.default_rng(seed)
    # grow the tree by attaching every new leaf to a new node on a random edge; edges as (u, v, length)
    def length():
        return int(rng.integers(1, 10))
    edges = [(0, n, length()), (1, n, length()), (2, n, length())]
    nodes = n + 1
    for leaf in range(3, n):
        u, v, _w = edges.pop(int(rng.integers(len(edges))))
        edges += [(u, nodes, length()), (nodes, v, length()), (leaf, nodes, length())]
        nodes += 1
    adj = {k: [] for k in range(nodes)}
    for u, v, w in edges:
        adj[u].append((v, w))
        adj[v].append((u, w))
    dist = np.zeros((n, n))
    for s in range(n):
        seen, stack = {s: 0}, [s]
        while stack:
            x = stack.pop()
            for y, w in adj[x]:
                if y not in seen:
                    seen[y] = seen[x] + w
                    stack.append(y)
        dist[s] = [seen[t] for t in range(n)]
    return np.array([dist[i, j] for i, j in combinations(range(n), 2)], dtype=np.float32)


def relabel(pred: np.ndarray, perm) -> np.ndarray:
    """The distance vector after sequence ``k`` takes the label ``perm[k]``; also the index map new pair <- old pair."""
    n = len(perm)
    index = {pair: k for k, pair in enumerate(combinations(range(n), 2))}
    out = np.empty_like(pred)
    where = np.empty(len(pred), dtype=np.int64)
    for (i, j), k in index.items():
        a, b = sorted((perm[i], perm[j]))
        out[index[a, b]] = pred[k]
        where[index[a, b]] = k
    return out, where


def check_delta_files(files, stem, pred, ids):
    """The three files of ``stem`` hold ``delta_scores`` of the statement for ``pred``."""
    from phyloformer_amd.phylip import vec_to_phylip
    n = len(ids)
    pair_sum, hist, flag = D.delta_py(pred, n)
    assert flag == 0
    s = D.delta_scores(pair_sum, hist, n)
    overall, quartets, names, per_taxon, relative = D.parse_delta_tsv(files[f"{stem}.delta.tsv"].decode())
    assert quartets == comb(n, 4) and names == list(ids)
    assert overall == float(f"{s.overall:.10f}")
    assert per_taxon.tolist() == [float(f"{x:.10f}") for x in s.taxon]
    assert relative.tolist() == [float(f"{x / s.taxon.mean():.10f}") for x in s.taxon]
    assert np.array_equal(D.parse_hist_tsv(files[f"{stem}.delta.hist.tsv"].decode()), hist)
    rows = files[f"{stem}.delta.hist.tsv"].decode().splitlines()
    assert rows[0].split("\t") == ["bin", "from", "to", "quartets", "share"] and len(rows) == 21
    assert rows[14].split("\t")[:3] == ["13", "0.6500", "0.7000"]
    assert sum(float(r.split("\t")[4]) for r in rows[1:]) == pytest.approx(1.0, abs=1e-8)
    assert files[f"{stem}.delta.phy"].decode() == vec_to_phylip(s.pair.astype(np.float32), ids)[1]
    return s
