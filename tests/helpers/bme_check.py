"""An independent check of balanced minimum-evolution trees, and the inputs the BME tests share.

The balanced length here is Pauplin's: ``L = sum_{i<j} d_ij 2^(1 - edges(i, j))`` with the edges counted on the unrooted
tree of a join table by breadth-first search - no subtree averages, nothing of ``phyloformer_amd/bme.py``."""
from collections import deque
from typing import Dict, List, Sequence, Set

import numpy as np


def adjacency(slots: Sequence[int], n: int) -> Dict[int, Set[int]]:
    """The unrooted tree of a join table: leaves ``0 .. n-1``, node ``n + t`` from join ``t``, the trifurcation last."""
    adj: Dict[int, Set[int]] = {v: set() for v in range(2 * n - 2)}
    cluster = list(range(n))
    for t in range(n - 3):
        a, b = int(slots[2 * t]), int(slots[2 * t + 1])
        for c in (cluster[a], cluster[b]):
            adj[n + t].add(c)
            adj[c].add(n + t)
        cluster[a] = n + t
    for s in slots[2 * (n - 3):]:
        adj[2 * n - 3].add(cluster[int(s)])
        adj[cluster[int(s)]].add(2 * n - 3)
    return adj


def pauplin_length(adj: Dict[int, Set[int]], d: np.ndarray) -> float:
    n = d.shape[0]
    total = 0.0
    for i in range(n):
        dist = {i: 0}
        todo = deque([i])
        while todo:
            v = todo.popleft()
            for u in adj[v]:
                if u not in dist:
                    dist[u] = dist[v] + 1
                    todo.append(u)
        for j in range(i + 1, n):
            total += float(d[i, j]) * 2.0 ** (1 - dist[j])
    return total


def nni_neighbours(adj: Dict[int, Set[int]], n: int):
    """Every tree one nearest-neighbour interchange away: ``2 (n - 3)`` adjacency maps."""
    for u in range(n, 2 * n - 2):
        for v in adj[u]:
            if v < n or v < u:
                continue
            b = sorted(adj[u] - {v})[1]
            for c in sorted(adj[v] - {u}):
                new = {k: set(s) for k, s in adj.items()}
                new[u].remove(b); new[b].remove(u); new[v].remove(c); new[c].remove(v)
                new[u].add(c); new[c].add(u); new[v].add(b); new[b].add(v)
                yield new


def splits_of(slots: Sequence[int], n: int) -> Set[frozenset]:
    """The internal splits of a join table, each as the side without leaf 0."""
    members: List[Set[int]] = [{i} for i in range(n)]
    out = set()
    for t in range(n - 3):
        a, b = int(slots[2 * t]), int(slots[2 * t + 1])
        members[a] = members[a] | members[b]
        side = members[a]
        out.add(frozenset(set(range(n)) - side if 0 in side else side))
    return out


def random_tree_distances(n: int, seed: int) -> np.ndarray:
    """float32 ``[P_n]``: the path lengths of a random binary tree on ``n`` leaves with branch lengths in (0.02, 0.5)."""
    rng = np.random.default_rng(seed)
    adj: Dict[int, Dict[int, float]] = {0: {}, 1: {}, 2: {}, n: {}}
    for leaf in range(3):
        w = float(rng.uniform(0.02, 0.5))
        adj[leaf][n] = adj[n][leaf] = w
    nxt = n + 1
    for leaf in range(3, n):                                    # a new leaf on a random edge
        edges = [(u, v) for u in adj for v in adj[u] if u < v]
        u, v = edges[int(rng.integers(len(edges)))]
        del adj[u][v], adj[v][u]
        adj[nxt], adj[leaf] = {}, {}
        for x in (u, v, leaf):
            w = float(rng.uniform(0.02, 0.5))
            adj[nxt][x] = adj[x][nxt] = w
        nxt += 1
    dm = np.zeros((n, n))
    for i in range(n):
        dist = {i: 0.0}
        todo = deque([i])
        while todo:
            v = todo.popleft()
            for u, w in adj[v].items():
                if u not in dist:
                    dist[u] = dist[v] + w
                    todo.append(u)
        dm[i] = [dist[j] for j in range(n)]
    return dm[np.triu_indices(n, 1)].astype(np.float32)


def caterpillar_slots(n: int) -> np.ndarray:
    """The join table of the caterpillar in index order: ``(0, 1), (0, 2), ...``, then ``0, n - 2, n - 1``."""
    return np.array([s for t in range(n - 3) for s in (0, t + 1)] + [0, n - 2, n - 1], dtype=np.int32)


def uniform_preds(n: int, seed: int, b: int = 1) -> np.ndarray:
    return np.random.default_rng(seed).uniform(0.01, 3.0, size=(b, n * (n - 1) // 2)).astype(np.float32)


def star_tie_preds(n: int = 40, seed: int = 2) -> np.ndarray:
    """float32 ``[P_n]``: ``d_ij = a_i + a_j`` with integer ``a`` below 2^23, exact in float32.  Every topology has the same
    balanced length, so every ``delta`` is 0 but for rounding - and from the caterpillar the subtree weights reach
    2^-37, so the sums round (integers of 24 bits times 2^-37 do not fit 53 bits) at about 1e-9, far above the
    threshold of 1e-12: an incrementally updated table and a from-scratch one disagree about which moves qualify.
    With ``n = 40, seed = 2`` the serial driver reports two from-scratch tables that resumed the search."""
    a = np.random.default_rng(seed).integers(1 << 20, 1 << 23, size=n).astype(np.float64)
    dm = a[:, None] + a[None, :]
    vec = dm[np.triu_indices(n, 1)].astype(np.float32)
    assert (vec.astype(np.float64) == dm[np.triu_indices(n, 1)]).all()
    return vec


def noisy_start(vec: np.ndarray, n: int, seed: int, noise: float = 0.2) -> np.ndarray:
    """A start some tens of moves away: the NJ table of the distances with multiplicative noise."""
    from phyloformer_amd import bme
    f = np.random.default_rng(seed).uniform(1 - noise, 1 + noise, size=vec.shape)
    return bme.nj_start(bme.matrix_of_preds((vec * f).astype(np.float32), n))
