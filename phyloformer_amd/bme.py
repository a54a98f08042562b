"""Balanced minimum-evolution refinement of a neighbour-joining tree by balanced nearest-neighbour interchanges (BNNI;
Desper & Gascuel 2002, the ``-n B`` search of FastME) for the ``--bme`` flag of the CLI.  DESIGN.md section 21.

This module is the readable statement of the algorithm and the yardstick of the native code (``csrc/pf_bme_host.h``,
``csrc/pf_bme.hip.h``): steepest descent, the whole table of balanced averages rebuilt from scratch at every step, in a
fixed summation order.  Pinned against FastME ``-m N -n B`` (tests/golden/fastme_nj_bnni.json, tests/test_bme.py).

**Tree.**  Leaves are ``0 .. N-1``; internal node ``N + t`` comes from join ``t`` of the start table; node ``2N - 3`` is
the trifurcation, and the tree is kept rooted there.  An edge carries the id of its child node (``2N - 3`` edges; the
internal ones are ``N .. 2N-4``).  Every edge has two directed subtrees: row ``e`` is the subtree below edge ``e``
(rooted at node ``e``), row ``2N - 3 + e`` everything beyond its parent end (rooted at ``parent[e]``).

**Balanced averages.**  ``w_X(i) = 2^-(edges from X's root node to leaf i)`` (0 outside ``X``),
``M[X][j] = sum_i w_X(i) d_ij`` (``i`` ascending, product and add rounded separately) and
``d_XY = sum_j w_Y(j) M[X][j]`` in numpy's pairwise order over all ``j < N`` (``csrc/pf_nj_host.h::pairwise_sum``).

**Moves.**  For internal edge ``c`` with parent ``p``: ``c1 < c2`` the children of ``c``, ``s`` the sibling of ``c``
(``p`` the root: the lower-numbered of the two other children, the higher one being ``A``'s root), ``A`` the rest beyond
``p``, ``B`` the subtree of ``s``.  Move ``k`` swaps ``s`` with ``c1`` (``k = 0``) or ``c2`` (``k = 1``); with ``C`` / ``D``
the swapped / unswapped child, ``delta = 0.5 ((d_AC + d_BD) - (d_AB + d_CD))`` - twice the change of the balanced tree
length, whose sign is all the search needs.  The minimum of the key ``(delta, c, k)`` is performed iff
``delta < -1e-12``; the search ends when no move qualifies, or with status ``capped`` after ``16 N`` moves.

**Lengths** (from the table of the final topology): internal edge ``0.25 (d_AC + d_AD + d_BC + d_BD) - 0.5 (d_AB +
d_CD)``, leaf edge ``0.5 (d_iA + d_iB - d_AB)``; ``tree_length`` is their sum in edge order.

**Output.**  A join table in ``nj.nj_joins``' form: the internal nodes in ascending order of (number of leaves, smallest
leaf) - children before parents -, each joining its two children; a cluster's slot is its smallest leaf, so the
cluster in slot ``a < b`` keeps slot ``a``; then the root's three children by ascending slot.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .nj import Final, Join, newick_of_joins, nj_joins

# From this many sequences on the CLI refines a launch's trees on the GPU thread (``Engine.nj_joins`` +
# ``Engine.bme_nni``) instead of on the writer threads' host code.  A measured constant (DESIGN.md section 21,
# tools/bme_bench.py, profiles/bme_bench.txt): the smallest measured N at which the device side takes at most half the
# host's time; None = the device path is off in the CLI (the API stays).
BME_DEVICE_MIN = 128

THRESHOLD = -1e-12          # a move is performed iff delta < THRESHOLD (absolute: substitutions per site)
OK, NONFINITE, CAPPED = 0, 1, 2


def step_cap(n: int) -> int:
    return 16 * n


class Tree:
    """``parent [2N-2]`` (-1 at the root) and ``children [2N-2][3]`` (-1 where absent; ascending) of the rooted tree."""

    def __init__(self, slots: Sequence[int], n: int):
        slots = [int(s) for s in slots]
        if n < 3 or len(slots) != 2 * (n - 3) + 3:
            raise ValueError(f"a join table of {n} sequences has {2 * (n - 3) + 3} slots")
        self.n = n
        self.root = 2 * n - 3
        self.parent = np.full(2 * n - 2, -1, dtype=np.int32)
        self.children = np.full((2 * n - 2, 3), -1, dtype=np.int32)
        cluster = list(range(n))
        for t in range(n - 3):
            a, b = slots[2 * t], slots[2 * t + 1]
            if not (0 <= a < n and 0 <= b < n) or a == b or cluster[a] < 0 or cluster[b] < 0:
                raise ValueError(f"invalid join table: join {t} of slots {a}, {b}")
            self._adopt(n + t, [cluster[a], cluster[b]])
            cluster[a], cluster[b] = n + t, -1
        last = slots[2 * (n - 3):]
        if any(not 0 <= s < n for s in last) or len(set(last)) != 3 or any(cluster[s] < 0 for s in last):
            raise ValueError(f"invalid join table: trifurcation of slots {last}")
        self._adopt(self.root, [cluster[s] for s in last])

    def _adopt(self, node: int, kids: List[int]):
        for k, c in enumerate(sorted(kids)):
            self.children[node, k] = c
            self.parent[c] = node

    def quartet(self, c: int) -> Tuple[int, int, int, int, int, int]:
        """Edge ``c`` (any edge but the root): ``(p, s, arow, aroot, c1, c2)`` - the parent, the sibling (``B``), the row
        and the root node of ``A``, and the children of ``c`` (-1 for a leaf)."""
        p = int(self.parent[c])
        others = [int(x) for x in self.children[p] if x >= 0 and x != c]
        if p == self.root:
            s, aroot = others
            arow = aroot
        else:
            s, aroot, arow = others[0], int(self.parent[p]), self.root + p
        return p, s, arow, aroot, int(self.children[c, 0]), int(self.children[c, 1])

    def swap(self, c: int, k: int):
        """Move ``k`` of internal edge ``c``: the sibling ``s`` and child ``k`` of ``c`` change places."""
        p, s, _arow, _aroot, c1, c2 = self.quartet(c)
        x, y = (c1, c2) if k == 0 else (c2, c1)
        self.parent[s], self.parent[x] = c, p
        self.children[c, :2] = sorted((s, y))
        kids = sorted([int(v) for v in self.children[p] if v >= 0 and v != s] + [x])
        self.children[p, :len(kids)] = kids

    def depths(self) -> np.ndarray:
        """``int16 [4N-6][2N-2]``: every node's distance in edges from the root node of every directed subtree, -1
        outside it."""
        n, root = self.n, self.root
        depth = np.full((2 * root, 2 * n - 2), -1, dtype=np.int16)
        order = [root]
        for v in order:                                         # parents before children
            order.extend(int(c) for c in self.children[v] if c >= 0)

        def hang(row, under):
            np.copyto(depth[row], depth[under] + 1, where=depth[under] >= 0)

        for v in reversed(order[1:]):                           # below edge v
            depth[v, v] = 0
            for c in self.children[v]:
                if c >= 0:
                    hang(v, c)
        for v in order[1:]:                                     # beyond the parent end of edge v
            p = int(self.parent[v])
            depth[root + v, p] = 0
            for c in self.children[p]:
                if c >= 0 and c != v:
                    hang(root + v, c)
            if p != root:
                hang(root + v, root + p)
        return depth


def matrix_of_preds(preds: np.ndarray, n: int) -> np.ndarray:
    """The symmetric float64 matrix of ``preds float32 [n (n - 1) / 2]`` as ``nj`` sees it (``vec_to_matrix``)."""
    from .phylip import vec_to_matrix
    return vec_to_matrix(np.asarray(preds, dtype=np.float32), n).astype(np.float64)


class Table:
    """The balanced averages of one topology, from scratch: ``q [2N-3][6]`` = ``d_AB, d_CD, d_A c1, d_A c2, d_B c1,
    d_B c2`` of every edge (a leaf edge: ``d_AB, -, d_A e, -, d_B e, -``), the two ``delta`` of every internal edge and
    the balanced length of every edge."""

    def __init__(self, d: np.ndarray, tree: Tree):
        n, root = tree.n, tree.root
        depth = tree.depths()[:, :n]
        w = np.where(depth >= 0, np.ldexp(1.0, -depth.astype(np.int32)), 0.0)
        m = np.zeros((2 * root, n))
        for i in range(n):
            m = m + w[:, i:i + 1] * d[i][None, :]
        xs, ys = np.zeros((root, 6), dtype=np.int64), np.zeros((root, 6), dtype=np.int64)
        use = np.zeros((root, 6), dtype=bool)
        for e in range(root):
            _p, s, arow, _aroot, c1, c2 = tree.quartet(e)
            if c1 < 0:
                xs[e], ys[e], use[e] = (arow, 0, arow, 0, s, 0), (s, 0, e, 0, e, 0), (True, False, True, False, True, False)
            else:
                xs[e], ys[e], use[e] = (arow, c1, arow, arow, s, s), (s, c2, c1, c2, c1, c2), True
        q = np.ascontiguousarray(w[ys.ravel()] * m[xs.ravel()]).sum(axis=1).reshape(root, 6)
        q[~use] = 0.0
        self.q = q
        ab_cd = q[:, 0] + q[:, 1]
        self.delta = np.stack([0.5 * ((q[:, 2] + q[:, 5]) - ab_cd), 0.5 * ((q[:, 3] + q[:, 4]) - ab_cd)], axis=1)
        self.delta[:n] = np.inf
        internal = 0.25 * (((q[:, 2] + q[:, 3]) + q[:, 4]) + q[:, 5]) - 0.5 * ab_cd
        leaf = 0.5 * ((q[:, 2] + q[:, 4]) - q[:, 0])
        self.lengths = np.where(np.arange(root) < n, leaf, internal)

    def best(self) -> Tuple[float, int, int, float]:
        """The minimum key ``(delta, c, k)`` and the second-smallest ``delta`` (inf when there is none)."""
        flat = self.delta.ravel()
        if flat.size == 0 or not np.isfinite(flat).any():
            return np.inf, -1, -1, np.inf
        i = int(np.argmin(flat))                                 # the first minimum: the smallest (c, k)
        rest = np.delete(flat, i)
        return float(flat[i]), i // 2, i % 2, float(rest.min()) if rest.size else np.inf

    def tree_length(self) -> float:
        total = 0.0
        for x in self.lengths:
            total += float(x)
        return total


def joins_of_tree(tree: Tree, lengths: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The join table ``(slots int32, lengths float64) [2 (N - 3) + 3]`` of a tree and its edge lengths."""
    n, root = tree.n, tree.root
    size = np.ones(2 * n - 2, dtype=np.int64)
    low = np.arange(2 * n - 2, dtype=np.int64)
    order = [root]
    for v in order:
        order.extend(int(c) for c in tree.children[v] if c >= 0)
    for v in reversed(order):
        if v >= n:
            kids = [int(c) for c in tree.children[v] if c >= 0]
            size[v], low[v] = sum(size[c] for c in kids), min(low[c] for c in kids)
    slots, out = [], []
    for v in sorted(range(n, root), key=lambda u: (size[u], low[u])) + [root]:
        for c in sorted((int(c) for c in tree.children[v] if c >= 0), key=lambda u: low[u]):
            slots.append(int(low[c]))
            out.append(float(lengths[c]))
    return np.array(slots, dtype=np.int32), np.array(out, dtype=np.float64)


def bme_nni(dm: np.ndarray, start_slots: Sequence[int], trace: Optional[list] = None):
    """BNNI from the tree of ``start_slots`` on the symmetric float64 ``dm``: ``(slots, lengths, steps, tree_length,
    status)``.  ``trace``, when a list, receives ``(delta, c, k, second-best delta)`` of every table."""
    d = np.array(dm, dtype=np.float64)
    n = d.shape[0]
    tree = Tree(start_slots, n)
    if not np.isfinite(d).all():
        t = 2 * (n - 3) + 3
        return np.zeros(t, dtype=np.int32), np.zeros(t), 0, 0.0, NONFINITE
    steps, status = 0, OK
    while True:
        table = Table(d, tree)
        delta, c, k, second = table.best()
        if trace is not None:
            trace.append((delta, c, k, second))
        if not delta < THRESHOLD:
            break
        if steps >= step_cap(n):
            status = CAPPED
            break
        tree.swap(c, k)
        steps += 1
    slots, lengths = joins_of_tree(tree, table.lengths)
    return slots, lengths, steps, table.tree_length(), status


def table_to_joins(slots: Sequence[int], lengths: Sequence[float]) -> Tuple[List[Join], Final]:
    t = (len(slots) - 3) // 2
    joins = [(int(slots[2 * s]), int(slots[2 * s + 1]), float(lengths[2 * s]), float(lengths[2 * s + 1])) for s in range(t)]
    i, j, k = (int(x) for x in slots[2 * t:])
    li, lj, lk = (float(x) for x in lengths[2 * t:])
    return joins, (i, j, k, li, lj, lk)


def nj_start(dm: np.ndarray) -> np.ndarray:
    """The slots of ``nj.nj_joins``' table of ``dm``."""
    joins, final = nj_joins(dm)
    return np.array([s for a, b, _la, _lb in joins for s in (a, b)] + list(final[:3]), dtype=np.int32)


def caterpillar_slots(n: int) -> np.ndarray:
    """A valid join table whatever the distances: ``(0, 1), (0, 2), ...``, then ``0, n - 2, n - 1``."""
    return np.array([s for t in range(n - 3) for s in (0, t + 1)] + [0, n - 2, n - 1], dtype=np.int32)


def bme_newick_py(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> str:
    """``<stem>.bme.nwk``: the NJ tree of ``preds float32 [P_n]`` refined by BNNI, with balanced branch lengths.  Fewer
    than four sequences have no internal edge to move and fewer than three no table: the NJ text (``n = 3``: with
    balanced lengths, which a star shares with NJ's formulas but not its roundings).  Non-finite distances: the NJ text."""
    return bme_tree_py(preds, ids, clamp_negative)[0]


def bme_tree_py(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> Tuple[str, int]:
    """``bme_newick_py``'s text and the number of moves behind it."""
    from .nj import neighbor_joining
    n = len(ids)
    dm = matrix_of_preds(preds, n)
    if n < 3 or not np.isfinite(dm).all():
        return neighbor_joining(dm, ids, clamp_negative), 0
    slots, lengths, steps, _length, _status = bme_nni(dm, nj_start(dm))
    return newick_of_joins(ids, *table_to_joins(slots, lengths), clamp_negative), steps
