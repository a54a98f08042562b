"""Query placement on the host: the host twins of ``csrc/pf_place.hip.h``, the least-squares placement of a query on
the backbone's tree and the writers of ``infer_alns.py --place Q``.

"Add one in", the mirror of leave-one-out (``taxa.py``).  An alignment of ``M`` rows is a backbone - its first ``N``
rows - and ``Q = M - N`` queries, its last rows, where ``mafft --add`` and its kin put them.  Phyloformer's distances are
context dependent, so a query's distances to the backbone change with whichever other queries share its forward: every
query is forwarded alone with the backbone.  Set ``q`` is ``join_query(idx, N, q)``, the rows ``(0, .., N - 1, N + q)``:
the query is its row ``N``.  With ``P_n = n (n - 1) / 2`` and ``pair_n`` the pair order of ``taxa.pair_index``:

    place[q][i] = sets[q][pair_{N+1}(i, N)]                                    query q's distance to backbone row i
    delta_q(i, j) = sets[q][pair_{N+1}(i, j)] - base[pair_N(i, j)]             over the P_N backbone pairs
    disturb[q]  = sqrt(mean delta_q^2)                                         how far q moves the backbone's own distances
    shift[q]    = mean delta_q                                                 signed
    joint[q]    = sqrt(mean_i (whole[pair_M(i, N + q)] - place[q][i])^2)       how far the OTHER queries move q's distances

They are descriptive, not a test statistic.

``ls_place`` puts a query on the tree by ordinary least squares (what APPLES calls OLS): on every edge the attachment
point ``x`` and the pendant length ``y`` that minimise the squared differences between the query's distances and the
tree's, the best edge wins.  ``graft`` writes the tree with the queries attached.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .treecmp import Node, parse_newick


def join_query(idx: np.ndarray, N: int, q: int) -> np.ndarray:
    """``uint8[M, L]`` (or ``[B, M, L]``) → ``uint8[N + 1, L]``: the backbone rows ``0 .. N - 1`` and query ``q`` (row
    ``N + q``) behind them - the host twin of the row table ``(0, .., N - 1, N + q)`` given to ``k_gather_taxa``."""
    idx = np.asarray(idx, dtype=np.uint8)
    N, q = int(N), int(q)
    if idx.ndim not in (2, 3):
        raise ValueError(f"idx must be [B, M, L] or [M, L], got shape {idx.shape}")
    M = idx.shape[-2]
    if N < 2 or not 0 <= q < M - N:
        raise ValueError(f"query {q} of a backbone of {N} needs N >= 2 and 0 <= q < M - N (M = {M})")
    return np.ascontiguousarray(np.concatenate([idx[..., :N, :], idx[..., N + q:N + q + 1, :]], axis=-2))


def _row_start(i, n):
    return i * (2 * n - i - 1) // 2


def place_stats(whole: np.ndarray, base: np.ndarray, sets: np.ndarray, N: int, Q: int):
    """``whole [..., P_M]``, ``base [..., P_N]``, ``sets [..., Q, P_{N+1}]`` → ``(place [..., Q, N], disturb [..., Q],
    shift [..., Q], joint [..., Q])``: the literal definitions in float64, rounded to float32 once (``place`` is a copy)."""
    N, Q = int(N), int(Q)
    M = N + Q
    w = np.asarray(whole)
    b = np.asarray(base)
    s = np.asarray(sets)
    if N < 2 or Q < 1:
        raise ValueError(f"placement needs N >= 2 and Q >= 1 (got N={N}, Q={Q})")
    if (w.shape[-1] != M * (M - 1) // 2 or b.shape[-1] != N * (N - 1) // 2 or s.ndim < 2 or
            s.shape[-2:] != (Q, (N + 1) * N // 2) or w.shape[:-1] != b.shape[:-1] or s.shape[:-2] != w.shape[:-1]):
        raise ValueError(f"shapes {w.shape}, {b.shape}, {s.shape} are not those of N={N}, Q={Q}")
    i = np.arange(N)
    last = _row_start(i, N + 1) + (N - i - 1)                       # pair_{N+1}(i, N)
    place = s[..., last]                                            # [..., Q, N]
    wq = np.stack([w[..., _row_start(i, M) + (N + q - i - 1)] for q in range(Q)], axis=-2)      # pair_M(i, N + q)
    joint = np.sqrt(((wq.astype(np.float64) - place.astype(np.float64)) ** 2).mean(axis=-1))
    iu, _ju = np.triu_indices(N, k=1)                               # pair p of N rows sits at p + i among N + 1
    delta = s[..., np.arange(iu.size) + iu].astype(np.float64) - b.astype(np.float64)[..., None, :]
    disturb = np.sqrt((delta ** 2).mean(axis=-1))
    shift = delta.mean(axis=-1)
    return (np.ascontiguousarray(place, dtype=np.float32), disturb.astype(np.float32), shift.astype(np.float32),
            joint.astype(np.float32))


# ---- least-squares placement -----------------------------------------------------------------------------------------

class Backbone:
    """A tree as ``ls_place`` sees it: unrooted, its leaves indexed by ``labels``.

    ``edges[k] = (u, v, length)`` in the order that breaks ties: nodes are numbered in preorder of the Newick text
    (children in written order) and every node but the root contributes the edge to its parent, ``u`` the parent, ``v``
    the node, in that numbering's order.  A root with exactly two children is no node of the unrooted tree: its two
    edges are ONE edge, the first of the list, ``u`` the first child, ``v`` the second, their lengths added.  ``x`` is
    measured from ``u``.  A missing length counts as 0, a negative one is an error."""

    def __init__(self, tree, labels: Sequence[str]):
        root = tree if isinstance(tree, Node) else parse_newick(tree.decode("utf8") if isinstance(tree, bytes) else tree)
        self.root = root
        self.labels = [str(x) for x in labels]
        index = {name: k for k, name in enumerate(self.labels)}
        if len(index) != len(self.labels):
            raise ValueError("duplicate labels")
        nodes: List[Node] = []
        parent: List[int] = []
        stack = [(root, -1)]
        while stack:                                               # preorder, children in written order
            n, p = stack.pop()
            nodes.append(n)
            parent.append(p)
            me = len(nodes) - 1
            stack.extend((c, me) for c in reversed(n.children))
        # (the stack pops a node's first child right after the node, but its later children only after the first
        # child's whole subtree: that is preorder)
        self.nodes, self.parent = nodes, parent
        n_nodes, N = len(nodes), len(self.labels)
        self.leaf_of = [-1] * n_nodes                              # node -> leaf index
        below = np.zeros((n_nodes, N), dtype=bool)
        for k in range(n_nodes - 1, -1, -1):                       # children have larger numbers than their parent
            if nodes[k].is_leaf():
                if nodes[k].name not in index:
                    raise ValueError(f"leaf {nodes[k].name!r} is not among the labels")
                self.leaf_of[k] = index[nodes[k].name]
                if below[:, self.leaf_of[k]].any():
                    raise ValueError(f"leaf {nodes[k].name!r} occurs twice")
                below[k, self.leaf_of[k]] = True
            if parent[k] >= 0:
                below[parent[k]] |= below[k]
        if root.is_leaf() or not below[0].all():
            raise ValueError("the tree must hold every label as a leaf")
        length = [0.0 if n.length is None else float(n.length) for n in nodes]
        if any(l < 0 for l in length[1:]):
            raise ValueError("negative branch length")
        self.merged_root = len(root.children) == 2
        self.edges: List[Tuple[int, int, float]] = []
        self.v_side: List[np.ndarray] = []                         # per edge: the leaves on v's side
        kids = [k for k in range(1, n_nodes) if parent[k] == 0]
        if self.merged_root:
            c1, c2 = kids
            self.edges.append((c1, c2, length[c1] + length[c2]))
            self.v_side.append(below[c2].copy())
            self.root_split = length[c1]                           # where the written root sits on that edge, from u
        for k in range(1, n_nodes):
            if self.merged_root and parent[k] == 0:
                continue
            self.edges.append((parent[k], k, length[k]))
            self.v_side.append(below[k].copy())
        # node-to-leaf path lengths D [node][leaf] over the unrooted tree
        adj: List[List[Tuple[int, float]]] = [[] for _ in range(n_nodes)]
        for u, v, l in self.edges:
            adj[u].append((v, l))
            adj[v].append((u, l))
        self.D = np.zeros((n_nodes, N))
        for k in range(n_nodes):
            if self.leaf_of[k] < 0:
                continue
            col = self.leaf_of[k]
            seen = {k}
            todo = [(k, 0.0)]
            while todo:
                a, da = todo.pop()
                self.D[a, col] = da
                for c, l in adj[a]:
                    if c not in seen:
                        seen.add(c)
                        todo.append((c, da + l))

    def edge_label(self, k: int, names: Optional[Sequence[str]] = None) -> str:
        """The sorted leaf set of edge ``k``'s smaller side (equal sizes: the lexicographically smaller list), joined by
        ``|``; ``names`` replaces the labels (the CLI's trees carry index labels)."""
        names = self.labels if names is None else [str(x) for x in names]
        side = self.v_side[k]
        a = sorted(names[i] for i in np.flatnonzero(side))
        b = sorted(names[i] for i in np.flatnonzero(~side))
        return "|".join(min((len(a), a), (len(b), b))[1])


class Placement(NamedTuple):
    edge: int          # index into Backbone.edges
    x: float           # attachment point, from the edge's u, in [0, length]
    pendant: float     # >= 0
    rss: float         # R, the sum of squared differences
    residual: float    # sqrt(R / N)


def fit_edge(bb: Backbone, k: int, d: np.ndarray) -> Tuple[float, float, float]:
    """``(x, y, R)`` of the least-squares attachment of distances ``d [N]`` to edge ``k``: the minimum of
    ``R = sum_i (d_i - y - (x + D(u, i) on u's side | length - x + D(v, i) on v's side))^2`` over ``0 <= x <= length``,
    ``y >= 0`` - a convex quadratic over a box: the unconstrained 2 x 2 solution if it lies inside, otherwise the best
    of the one-dimensional minima on the sides ``x = 0``, ``x = length``, ``y = 0`` (each clipped to its side)."""
    u, v, ell = bb.edges[k]
    d = np.asarray(d, dtype=np.float64)
    vs = bb.v_side[k]
    # residual_i = c_i - y - s_i x
    c = np.where(vs, d - bb.D[v] - ell, d - bb.D[u])
    s = np.where(vs, -1.0, 1.0)
    n = float(d.size)
    S, C, Sc = float(s.sum()), float(c.sum()), float((s * c).sum())

    def rss(x, y):
        r = c - y - s * x
        return float((r * r).sum())

    det = n * n - S * S                                            # 4 n_u n_v > 0: both sides hold a leaf
    x0, y0 = (n * Sc - S * C) / det, (n * C - S * Sc) / det
    if 0.0 <= x0 <= ell and y0 >= 0.0:
        return x0, y0, rss(x0, y0)
    cands = [(0.0, max(0.0, C / n)), (ell, max(0.0, (C - S * ell) / n)), (min(max(Sc / n, 0.0), ell), 0.0)]
    return min(((x, y, rss(x, y)) for x, y in cands), key=lambda t: t[2])


def ls_place(bb: Backbone, d: np.ndarray) -> Placement:
    """The least-squares placement of a query with distances ``d [N]`` (leaf order: ``bb.labels``): ``fit_edge`` on every
    edge, the smallest ``R`` wins, ties go to the first edge in the order of ``Backbone.edges``.  O(N^2) per query."""
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    if d.size != len(bb.labels):
        raise ValueError(f"{d.size} distances for {len(bb.labels)} leaves")
    best = None
    for k in range(len(bb.edges)):
        x, y, r = fit_edge(bb, k, d)
        if best is None or r < best.rss:
            best = Placement(k, x, y, r, float(np.sqrt(r / d.size)))
    return best


def _fmt(x: float) -> str:
    return repr(float(x))


def graft(bb: Backbone, placements: Sequence[Placement], query_names: Sequence[str], names: Optional[Sequence[str]] = None) -> str:
    """The backbone with every query attached where its placement says, each placed independently (Newick, terminated by
    ``;`` and a newline).  Several queries on one edge sit in the order of ``x``, then of their index; a query at ``x``
    splits the edge into ``x`` and ``length - x``.  The written root stays where it was: on a merged root edge a query
    with ``x`` up to the first child's length hangs on the first child's edge, the others on the second's.  ``names``
    replaces the backbone's labels."""
    names = bb.labels if names is None else [str(x) for x in names]
    per_edge: dict = {}
    for qi, p in enumerate(placements):
        per_edge.setdefault(p.edge, []).append((p.x, qi))
    edge_of = {v: k for k, (u, v, l) in enumerate(bb.edges)}
    number = {id(n): k for k, n in enumerate(bb.nodes)}

    def chain(sub: str, length: float, atts: List[Tuple[float, int]]) -> str:
        """``sub`` at the far end of an edge of ``length``, the queries ``atts`` = (distance from the near end, index),
        ascending, on it."""
        end = length
        for t, qi in reversed(atts):
            sub = f"({sub}:{_fmt(end - t)},{query_names[qi]}:{_fmt(placements[qi].pendant)})"
            end = t
        return f"{sub}:{_fmt(end)}"

    def text(n: Node) -> str:
        if n.is_leaf():
            return names[bb.leaf_of[number[id(n)]]]
        return "(" + ",".join(branch(c) for c in n.children) + ")"

    def branch(c: Node) -> str:
        k = number[id(c)]
        length = 0.0 if c.length is None else float(c.length)
        if bb.merged_root and bb.parent[k] == 0:
            atts = sorted(per_edge.get(0, []))
            u, v, ell = bb.edges[0]
            if k == u:                                             # x runs from u up to the written root
                return chain(text(c), length, [(length - x, qi) for x, qi in reversed(atts) if x <= bb.root_split])
            return chain(text(c), length, [(x - bb.root_split, qi) for x, qi in atts if x > bb.root_split])
        return chain(text(c), length, sorted(per_edge.get(edge_of[k], [])))

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        return text(bb.root) + ";\n"
    finally:
        sys.setrecursionlimit(old)


def prune_leaves(root: Node, drop: Sequence[str]) -> Node:
    """A copy of the tree without the leaves ``drop``: inner nodes left without a leaf go too, a node left with one child
    is merged with it (lengths added; at the root the child becomes the root)."""
    gone = set(drop)

    def copy(n: Node) -> Optional[Node]:
        if n.is_leaf():
            return None if n.name in gone else Node(n.name, n.length)
        kids = [k for k in (copy(c) for c in n.children) if k is not None]
        if not kids:
            return None
        if len(kids) == 1:
            only = kids[0]
            only.length = (only.length or 0.0) + (n.length or 0.0)
            return only
        out = Node(n.name, n.length)
        out.children = kids
        return out

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        out = copy(root)
    finally:
        sys.setrecursionlimit(old)
    if out is None:
        raise ValueError("every leaf was pruned")
    out.length = None
    return out


# ---- writers ---------------------------------------------------------------------------------------------------------

TSV_COLUMNS = ("index", "id", "nearest", "nearest_distance", "disturb", "shift", "joint")
TREE_COLUMNS = ("edge", "x", "pendant", "residual")


def place_dist_tsv(backbone_ids: Sequence[str], query_ids: Sequence[str], place: np.ndarray) -> str:
    """``<stem>.place.dist.tsv``: header ``query`` and the ``N`` backbone ids, one row per query: its id and its ``N``
    distances in the number format of ``<stem>.phy``."""
    pl = np.asarray(place, np.float64).reshape(len(query_ids), len(backbone_ids))
    rows = ["\t".join(["query"] + [str(i) for i in backbone_ids]) + "\n"]
    for qid, row in zip(query_ids, pl):
        rows.append("\t".join([str(qid)] + [f"{float(v):.10f}" for v in row]) + "\n")
    return "".join(rows)


def place_tsv(backbone_ids: Sequence[str], query_ids: Sequence[str], place: np.ndarray, disturb: np.ndarray, shift: np.ndarray,
              joint: np.ndarray, tree: Optional[Sequence[Tuple[str, object, object, object]]] = None) -> str:
    """``<stem>.place.tsv``: header ``index id nearest nearest_distance disturb shift joint`` (with ``tree`` also ``edge x
    pendant residual``), one row per query; ``index`` is the query's 0-based row in the file, ``nearest`` the backbone id
    of its smallest distance (the first on ties).  Numbers have the format of ``<stem>.phy``; ``tree[q]`` holds
    ``(edge label, x, pendant, residual)``, numbers or ``"NA"``."""
    N, Q = len(backbone_ids), len(query_ids)
    pl = np.asarray(place, np.float64).reshape(Q, N)
    cols = [np.asarray(a, np.float64).reshape(Q) for a in (disturb, shift, joint)]
    rows = ["\t".join(TSV_COLUMNS + (TREE_COLUMNS if tree is not None else ())) + "\n"]
    for q in range(Q):
        near = int(np.argmin(pl[q]))
        row = [str(N + q), str(query_ids[q]), str(backbone_ids[near]), f"{float(pl[q, near]):.10f}"]
        row += [f"{float(c[q]):.10f}" for c in cols]
        if tree is not None:
            row += [v if isinstance(v, str) else f"{float(v):.10f}" for v in tree[q]]
        rows.append("\t".join(row) + "\n")
    return "".join(rows)
