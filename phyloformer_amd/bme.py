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

**Balanced SPR** (the ``-s`` search of FastME, ``--spr``) is the second search on the same tree, rows,
averages, lengths and output: ``bme_spr``, whose docstring defines its pair table, candidates and rule.

**Output.**  A join table in ``nj.nj_joins``' form: the internal nodes in ascending order of (number of leaves, smallest
leaf) - children before parents -, each joining its two children; a cluster's slot is its smallest leaf, so the
cluster in slot ``a < b`` keeps slot ``a``; then the root's three children by ascending slot.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .nj import Final, Join, newick_of_joins, nj_joins, table_of_joins

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


def balanced_rows(d: np.ndarray, tree: Tree) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``depth int16 [4N-6][2N-2]``, ``w float64 [4N-6][N]`` and ``M float64 [4N-6][N]`` of one topology, from scratch."""
    n, root = tree.n, tree.root
    depth = tree.depths()
    leaf = depth[:, :n]
    w = np.where(leaf >= 0, np.ldexp(1.0, -leaf.astype(np.int32)), 0.0)
    m = np.zeros((2 * root, n))
    for i in range(n):
        m = m + w[:, i:i + 1] * d[i][None, :]
    return depth, w, m


class Table:
    """The balanced averages of one topology, from scratch: ``q [2N-3][6]`` = ``d_AB, d_CD, d_A c1, d_A c2, d_B c1,
    d_B c2`` of every edge (a leaf edge: ``d_AB, -, d_A e, -, d_B e, -``), the two ``delta`` of every internal edge and
    the balanced length of every edge."""

    def __init__(self, d: np.ndarray, tree: Tree):
        n, root = tree.n, tree.root
        _depth, w, m = balanced_rows(d, tree)
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
    return table_of_joins(*nj_joins(dm))[0]


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


# ---- balanced subtree pruning and regrafting (``--spr``) ---------------------------------------

# From this many sequences on the CLI refines a launch's trees on the GPU thread (``Engine.nj_joins`` +
# ``Engine.bme_spr``).  A measured constant by ``BME_DEVICE_MIN``'s rule (tools/spr_bench.py,
# profiles/spr_bench.txt); None = the device path is off in the CLI (the API stays).
SPR_DEVICE_MIN = 64


def neighbours(tree: Tree, u: int) -> List[int]:
    """The neighbours of node ``u``: its children in ascending order, then its parent."""
    out = [int(c) for c in tree.children[u] if c >= 0]
    if u != tree.root:
        out.append(int(tree.parent[u]))
    return out


def row_through(tree: Tree, v: int, u: int) -> int:
    """The row of the directed subtree through neighbour ``v`` of node ``u``, away from ``u``."""
    return v if int(tree.parent[v]) == u else tree.root + u


class PairTable:
    """``T float64 [4N-6][4N-6]`` of one topology, from scratch: ``T[X][Y] = d_XY`` in the module's one definition
    (``sum_j w_Y(j) M[X][j]`` over all ``j < N`` in ``pairwise_sum``'s order) for rows without a common leaf, 0.0 where
    they share one (never read)."""

    def __init__(self, d: np.ndarray, tree: Tree):
        depth, w, m = balanced_rows(d, tree)
        inside = (depth[:, :tree.n] >= 0).astype(np.int32)
        t = np.empty((2 * tree.root, 2 * tree.root))
        for x in range(2 * tree.root):
            t[x] = np.ascontiguousarray(w * m[x][None, :]).sum(axis=1)
        t[(inside @ inside.T) > 0] = 0.0
        self.depth, self.t = depth, t


def spr_candidates(t: Sequence[Sequence[float]], tree: Tree):
    """Every candidate of ``bme_spr``'s docstring as ``(dL, S row, target edge id, path)``, ``path = (u_1, ..., u_i,
    t)``; ``t`` is ``PairTable.t`` (or its ``tolist()``)."""
    n, root = tree.n, tree.root
    for srow in range(2 * root):
        e = srow if srow < root else srow - root
        snode, a = (e, int(tree.parent[e])) if srow < root else (int(tree.parent[e]), e)
        if a < n:
            continue
        others = [v for v in neighbours(tree, a) if v != snode]
        for n1, n2 in (others, others[::-1]):
            r = row_through(tree, n2, a)
            todo = [(n1, a, 1, t[r][srow], 0.0, (n1,))]
            while todo:
                u, prev, i, drs, acc, path = todo.pop()
                if u < n:
                    continue
                forward = [v for v in neighbours(tree, u) if v != prev]
                b = row_through(tree, prev, u)
                for nxt, other in (forward, forward[::-1]):
                    x, f = row_through(tree, other, u), row_through(tree, nxt, u)
                    drx = t[b][x] + float(np.ldexp(1.0, -i)) * (t[r][x] - t[srow][x])
                    total = acc + 0.25 * ((drx + t[srow][f]) - (drs + t[x][f]))
                    yield total, srow, (nxt if int(tree.parent[nxt]) == u else u), path + (nxt,)
                    todo.append((nxt, u, i + 1, 0.5 * drs + 0.5 * t[x][srow], total, path + (nxt,)))


def spr_move(tree: Tree, srow: int, path: Sequence[int]):
    """Carries out the candidate ``(S row, path)`` as its ``len(path) - 1`` calls of ``Tree.swap``: interchange ``j``
    goes across the edge between ``S``'s attachment node ``v`` at that time and ``u_j`` and lets ``S`` and ``X_j``
    change places.  ``Tree.swap(c, k)`` moves the sibling block ``s`` of ``Tree.quartet(c)``; where ``S`` or ``X_j`` is
    the block ``A`` instead, the same unrooted tree comes from letting ``s`` and the other child of ``c`` change places.
    This fixes the node numbers of the moved tree, which later ties are broken by."""
    root = tree.root
    e = srow if srow < root else srow - root
    for u, nxt in zip(path[:-1], path[1:]):
        v = int(tree.parent[e]) if srow < root else e
        if int(tree.parent[u]) == v:                  # down: S stands beside edge u as s or as A, X_j is a child of u
            _p, s, _arow, _aroot, c1, _c2 = tree.quartet(u)
            k_next = 0 if c1 == nxt else 1
            tree.swap(u, 1 - k_next if (srow < root and s == e) else k_next)
        else:                                         # up: S is child e of v, X_j stands beside edge v as s or as A
            _p, s, _arow, _aroot, c1, _c2 = tree.quartet(v)
            k_e = 0 if c1 == e else 1
            tree.swap(v, k_e if nxt != s else 1 - k_e)


def bme_spr(dm: np.ndarray, start_slots: Sequence[int], trace: Optional[list] = None):
    """Balanced SPR (FastME's ``-s`` search) from the tree of ``start_slots`` on the symmetric float64 ``dm``:
    ``(slots, lengths, steps, tree_length, status)``.  ``trace``, when a list, receives ``(dL, S row, target edge id,
    path)`` of every table's best candidate (``(inf, -1, -1, ())`` when there is none).

    **Pair table.**  ``T[X][Y] = sum_j w_Y(j) M[X][j]`` for directed subtrees without a common leaf (``PairTable``): the
    ``d_XY`` of the module docstring.  ``T[X][Y]`` and ``T[Y][X]`` differ in roundings; every term below reads the
    orientation written.

    **Candidates.**  The pruned subtree ``S`` is any row; its attachment node ``a`` (row ``e``: ``parent[e]``; row
    ``2N - 3 + e``: node ``e``, which has to be internal) has two other neighbours.  Moving towards one of them, ``n1``:
    ``R`` is the directed subtree through the other, ``n2``, away from ``a``; the path is ``u_0 = a, u_1 = n1, u_2, ...``.
    At path node ``u_i`` with ``t`` one of its two forward neighbours, ``F_i`` is the directed subtree through ``t``,
    ``X_i`` the one through the other forward neighbour and ``B_i`` the one through ``u_{i-1}`` (it contains ``S``), all
    away from ``u_i``.  Regrafting ``S`` onto edge ``(u_i, t)`` changes the balanced tree length by

        dRX_i = T[B_i][X_i] + 2^-i (T[R][X_i] - T[S][X_i])
        dRS_1 = T[R][S];   dRS_{i+1} = 0.5 dRS_i + 0.5 T[X_i][S]
        term_i = 0.25 ((dRX_i + T[S][F_i]) - (dRS_i + T[X_i][F_i]))
        dL = term_1 + ... + term_i        (added in path order, from 0.0)

    where the terms ``j < i`` are those of the path itself (``t = u_{j+1}``): the move is ``i`` successive NNIs, and
    ``dRX_i`` is the average between ``X_i`` and the balanced merge of ``R, X_1 .. X_{i-1}``.  ``4 (N - 2) (N - 3)``
    candidates, ``2 (N - 3) (2N - 7)`` distinct trees.

    **Rule.**  The minimum of the key ``(dL, S row, target edge id)`` is performed iff ``dL < THRESHOLD``.  (``S`` and
    the target edge fix the side of ``a`` the path leaves by, so a further key component for it would never decide.)
    ``dL`` is the change of the length itself, BNNI's ``delta`` twice that: the same ``THRESHOLD`` stands for half the
    change here.  The move is carried out by ``spr_move``.  The search ends when no candidate qualifies, or with status
    ``CAPPED`` after ``step_cap(N)`` moves.  Every step forms ``depth``, ``M`` and ``T`` from scratch.

    **Lengths**, ``tree_length`` and the output table come from ``Table`` of the final topology, as ``bme_nni``'s: the
    same topology gives the same bits whichever search found it."""
    d = np.array(dm, dtype=np.float64)
    n = d.shape[0]
    tree = Tree(start_slots, n)
    if not np.isfinite(d).all():
        t = 2 * (n - 3) + 3
        return np.zeros(t, dtype=np.int32), np.zeros(t), 0, 0.0, NONFINITE
    steps, status = 0, OK
    while True:
        best = min(spr_candidates(PairTable(d, tree).t.tolist(), tree), key=lambda c: c[:3], default=(np.inf, -1, -1, ()))
        if trace is not None:
            trace.append(best)
        if not best[0] < THRESHOLD:
            break
        if steps >= step_cap(n):
            status = CAPPED
            break
        spr_move(tree, best[1], best[3])
        steps += 1
    table = Table(d, tree)
    slots, lengths = joins_of_tree(tree, table.lengths)
    return slots, lengths, steps, table.tree_length(), status


def spr_newick_py(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> str:
    """``<stem>.spr.nwk``: the NJ tree of ``preds float32 [P_n]`` refined by balanced SPR moves, with balanced branch
    lengths.  The small and the non-finite cases are ``bme_newick_py``'s."""
    return spr_tree_py(preds, ids, clamp_negative)[0]


def spr_tree_py(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> Tuple[str, int]:
    """``spr_newick_py``'s text and the number of moves behind it."""
    from .nj import neighbor_joining
    n = len(ids)
    dm = matrix_of_preds(preds, n)
    if n < 3 or not np.isfinite(dm).all():
        return neighbor_joining(dm, ids, clamp_negative), 0
    slots, lengths, steps, _length, _status = bme_spr(dm, nj_start(dm))
    return newick_of_joins(ids, *table_to_joins(slots, lengths), clamp_negative), steps
