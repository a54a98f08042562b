"""What the balanced-SPR tests and the generator of their goldens share: the harder distance matrices, and subtree
pruning and regrafting on the plain adjacency of ``bme_check`` - nothing of ``phyloformer_amd/bme.py``."""
from typing import Dict, Iterator, List, Set, Tuple

import numpy as np

from . import bme_check as bc

UNIFORM = ((40, 5), (40, 6), (40, 7), (30, 8), (50, 9))
NOISY = ((40, 4), (50, 5), (60, 6))


def noisy_tree_preds(n: int, seed: int) -> np.ndarray:
    """float32 ``[P_n]``: ``random_tree_distances(n, seed)`` times log-normal noise ``exp(N(0, 0.3))``."""
    vec = bc.random_tree_distances(n, seed)
    noise = np.exp(np.random.default_rng(seed).normal(0.0, 0.3, size=vec.shape))
    return (vec * noise).astype(np.float32)


def harder_cases() -> List[Tuple[str, List[str], np.ndarray]]:
    """``(label, ids, float32 [P_n])`` of the eight matrices beside the 20 test alignments; sequences are ``T0 ...``."""
    out = [(f"uniform_preds({n}, {seed})", bc.uniform_preds(n, seed)[0]) for n, seed in UNIFORM]
    out += [(f"noisy_tree_preds({n}, {seed})", noisy_tree_preds(n, seed)) for n, seed in NOISY]
    return [(label, [f"T{i}" for i in range(int(round((1 + (1 + 8 * vec.size) ** 0.5) / 2)))], vec) for label, vec in out]


def regraft(adj: Dict[int, Set[int]], s: int, a: int, u: int, t: int) -> Dict[int, Set[int]]:
    """The subtree through neighbour ``s`` of node ``a`` pruned and regrafted onto edge ``(u, t)``: ``a``'s two other
    neighbours are joined, and ``a`` comes to stand on the edge."""
    new = {k: set(v) for k, v in adj.items()}
    n1, n2 = sorted(new[a] - {s})
    new[n1].discard(a); new[n2].discard(a); new[n1].add(n2); new[n2].add(n1)
    new[u].discard(t); new[t].discard(u)
    new[a] = {s, u, t}; new[u].add(a); new[t].add(a)
    return new


def side_of(adj: Dict[int, Set[int]], v: int, frm: int) -> Set[int]:
    """The nodes reached from ``v`` without passing ``frm``."""
    seen, todo = {v}, [v]
    while todo:
        x = todo.pop()
        for y in adj[x]:
            if y not in seen and not (x == v and y == frm):
                seen.add(y)
                todo.append(y)
    return seen


def spr_neighbours(adj: Dict[int, Set[int]], n: int) -> Iterator[Dict[int, Set[int]]]:
    """Every tree one subtree pruning and regrafting away, by brute force: ``4 (n - 2) (n - 3)`` adjacency maps (each
    of the ``2 (n - 3) (2n - 7)`` distinct trees at least once)."""
    for a in range(n, 2 * n - 2):
        for s in sorted(adj[a]):
            inside = side_of(adj, s, a) | {a}
            for u in sorted(set(adj) - inside):
                for t in sorted(adj[u] - inside):
                    if u < t:
                        yield regraft(adj, s, a, u, t)


def internal_splits(adj: Dict[int, Set[int]], n: int) -> frozenset:
    """The internal splits of an adjacency map, each as the side without leaf 0 (``bme_check.splits_of``'s form)."""
    out = set()
    for a in range(n, 2 * n - 2):
        for b in adj[a]:
            if b > a:
                leaves = frozenset(x for x in side_of(adj, a, b) if x < n)
                out.add(frozenset(range(n)) - leaves if 0 in leaves else leaves)
    return frozenset(out)
