"""Distances between trees on one set of sequences: shared splits (Robinson-Foulds), the Kuhner-Felsenstein branch score
and weighted RF, for the ``--treedist`` and ``--treedist-ref`` flags of the CLI (``scheduler.DirectoryRunner``).  DESIGN.md section 35.

This module is the readable statement and the yardstick of the native code (``csrc/pf_treedist_host.h``,
``csrc/pf_treedist.hip.h``): brute force, Python ints as bitsets, in the style of ``supports.py`` and ``consensus.py``.

**Inputs.**  One source: ``K >= 1`` join tables ``slots int32 [K][T]``, ``T = 2 (N - 3) + 3``, ``N >= 4``; optionally their
lengths ``float64 [K][T]`` and flags ``[K]``.  A flagged tree has no tree: its table is never read.

**Splits and lengths.**  The splits of a table are ``supports.table_splits`` (``N - 3`` per tree, the side without sequence
0, distinct within a tree).  The lengths sit where ``consensus.branch_positions`` says: the branch above join ``t``'s cluster
at the first ``p > 2 t + 1`` with ``slots[p] == slots[2 t]`` (``l(t)``), the branch of leaf ``x`` at the first ``p`` with
``slots[p] == x`` (``l(leaf x)``).

**A pair** ``i < j`` of unflagged trees walks one list of ``U = 3 N - 6`` terms ``d_u``:

* A, ``u = t``, ``t = 0 .. N - 4``: ``d = l_i(t) - b`` with ``b`` the length of the same split in tree ``j``, or ``+0.0`` if
  ``j`` lacks it; ``shared`` counts the hits;
* B, ``u = N - 3 + t``: ``d = 0.0 - l_j(t)`` if tree ``i`` lacks split ``t`` of tree ``j``, else ``+0.0``;
* C, ``u = 2 N - 6 + x``, ``x = 0 .. N - 1``: ``d = l_i(leaf x) - l_j(leaf x)``.

**Sums**, in section 32's order: 64 accumulators from ``+0.0``, ``acc[l] += term`` over ``u = l, l + 64, ...`` ascending, then
``acc[l] += acc[l + s]`` for ``l < s``, ``s`` = 32 .. 1 - once with the terms ``d * d``, once with ``|d|``.  Every product and
every sum is rounded where it is written (no contraction), so the device, its serial twin and this statement agree bit
for bit.

**Results**, mirrored to ``(j, i)``: ``shared int32 [K][K]`` (``RF = 2 (N - 3) - 2 shared``, ``nRF = RF / (2 (N - 3))``),
``kf float64 [K][K] = sqrt(acc[0])`` of the squares (the Kuhner-Felsenstein branch score) and ``wrf float64 [K][K]`` =
``acc[0]`` of the magnitudes (weighted RF).  The diagonal is ``N - 3`` and ``+0.0``; a pair with a flagged tree - a flagged
tree's diagonal too - is -1 and NaN.  Without lengths only ``shared`` is computed.

**Status.**  0; 1 where an unflagged table is no join table - every result of the source is then zero.  (2, the native
hash table's failure, does not exist here.)
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .consensus import branch_positions
from .supports import table_splits

# From this many sequences on the CLI compares a launch's written kinds (and the tree of --treedist-ref) on the GPU thread
# (``Engine.join_distances``) instead of on the writer threads' host side; None = the device path is off in the CLI (the API
# stays).  A measured constant by ``bme.BME_DEVICE_MIN``'s rule (tools/treedist_bench.py,
# profiles/treedist_bench.txt): the smallest measured N at which the engine call takes at most half the twin's time in every
# mix of trees, at K = 7 trees (1.3 to 2.5 times at 1,024; 5.5 times at 4,096).
TREEDIST_DEVICE_MIN = 4096
# The same for the NJ tree with its replicates, beside ``Bootstrap._extend``'s device calls, from ``TREEDIST_REPS_TREES`` trees
# (R + 1) on: the K = 101 lines, where the engine call is 13 times the twin's speed already at N = 20.  Fewer trees go by
# ``TREEDIST_DEVICE_MIN``, the K = 7 lines.
TREEDIST_REPS_DEVICE_MIN = 20
TREEDIST_REPS_TREES = 101

LANES = 64
MIN_SEQS = 4
NAN = float("nan")
COLUMNS = ("a", "b", "rf", "nrf", "wrf", "kf", "note")
FEW_SEQUENCES = "fewer than four sequences"
NOT_FINITE = "distances are not finite"
# the refusals of --treedist, in the wording of treekinds.refusals
NEEDS_TREES = "--treedist compares the trees of --trees: give -t as well"
SHARD_SITES = "--treedist cannot be combined with --shard sites: the site-sharded runner writes NJ trees only"
NOTHING_TO_COMPARE = ("--treedist has nothing to compare: only the NJ tree is written; --bme, --spr and --bionj write a second "
                      "tree, --treedist-ref DIR names one, --bootstrap R makes R replicate trees")


class Distances(NamedTuple):
    """One source's matrices (module docstring); ``kf`` and ``wrf`` are None without lengths."""
    shared: np.ndarray
    kf: Optional[np.ndarray]
    wrf: Optional[np.ndarray]
    status: int


def lane_sum(terms: Sequence[float]) -> float:
    """The sum of ``terms`` in the order of the module docstring."""
    acc = [0.0] * LANES
    for u, x in enumerate(terms):
        acc[u % LANES] = acc[u % LANES] + x
    s = LANES // 2
    while s:
        for l in range(s):
            acc[l] = acc[l] + acc[l + s]
        s //= 2
    return acc[0]


def pair_terms(splits_i, inner_i, leaf_i, splits_j, inner_j, leaf_j):
    """``(shared, [d_u])`` of one pair: the splits, the lengths of their branches and the leaves' lengths of both trees."""
    where_j = {s: t for t, s in enumerate(splits_j)}
    have_i = set(splits_i)
    hits = sum(s in where_j for s in splits_i)
    a = [inner_i[t] - (inner_j[where_j[s]] if s in where_j else 0.0) for t, s in enumerate(splits_i)]
    b = [0.0 if s in have_i else 0.0 - inner_j[t] for t, s in enumerate(splits_j)]
    c = [x - y for x, y in zip(leaf_i, leaf_j)]
    return hits, a + b + c


def join_distances_py(slots: Sequence[Sequence[int]], lengths: Optional[Sequence[Sequence[float]]], flag: Optional[Sequence[bool]],
                      n: int) -> Distances:
    """One source's tree distances (module docstring)."""
    K = len(slots)
    if K < 1:
        raise ValueError("tree distances need K >= 1 trees")
    if n < MIN_SEQS:
        raise ValueError(f"tree distances need N >= 4 sequences (got {n}): a tree of 3 has no split")
    flags = [False] * K if flag is None else [bool(f) for f in flag]
    if len(flags) != K or (lengths is not None and len(lengths) != K):
        raise ValueError(f"expected {K} flags and length rows")
    with_lengths = lengths is not None
    shared = np.zeros((K, K), dtype=np.int32)
    kf = np.zeros((K, K), dtype=np.float64) if with_lengths else None
    wrf = np.zeros((K, K), dtype=np.float64) if with_lengths else None
    try:
        trees = [None if f else table_splits(s, n) for s, f in zip(slots, flags)]
    except ValueError:
        return Distances(shared, kf, wrf, 1)
    inner: List[Optional[list]] = [None] * K
    leaf: List[Optional[list]] = [None] * K
    for k, splits in enumerate(trees):
        if splits is None:
            continue
        assert len(set(splits)) == n - 3
        if with_lengths:
            above, leaf_pos = branch_positions(slots[k], n)
            row = [float(x) for x in lengths[k]]
            inner[k], leaf[k] = [row[p] for p in above], [row[p] for p in leaf_pos]
        else:
            inner[k], leaf[k] = [0.0] * (n - 3), [0.0] * n
    for i in range(K):
        for j in range(i, K):
            if trees[i] is None or trees[j] is None:
                s, q, w = -1, NAN, NAN
            elif i == j:
                s, q, w = n - 3, 0.0, 0.0
            else:
                s, d = pair_terms(trees[i], inner[i], leaf[i], trees[j], inner[j], leaf[j])
                if with_lengths:
                    q, w = math.sqrt(lane_sum([x * x for x in d])), lane_sum([abs(x) for x in d])
            shared[i, j] = shared[j, i] = s
            if with_lengths:
                kf[i, j] = kf[j, i] = q
                wrf[i, j] = wrf[j, i] = w
    return Distances(shared, kf, wrf, 0)


def join_distances_batch_py(slots, lengths=None, flag=None):
    """``Engine.join_distances`` by the statement: ``[B, K, T]`` (or ``[K, T]``) → ``(shared, kf, wrf, status)``."""
    from .treearrays import distance_arrays, unbatched
    s, l, f, (b, k, n), single = distance_arrays(slots, lengths, flag)
    res = [join_distances_py(s[i], None if l is None else l[i], None if f is None else f[i], n) for i in range(b)]
    out = (np.stack([r.shared for r in res]), None if l is None else np.stack([r.kf for r in res]),
           None if l is None else np.stack([r.wrf for r in res]), np.array([r.status for r in res], dtype=np.uint8))
    return unbatched(out, single)


def reps_minimum(trees: int) -> Optional[int]:
    """The threshold of the replicate call over ``trees`` = R + 1 trees, as it is now."""
    return TREEDIST_REPS_DEVICE_MIN if trees >= TREEDIST_REPS_TREES else TREEDIST_DEVICE_MIN


def rf_of(shared: int, n: int) -> int:
    return 2 * (n - 3) - 2 * int(shared)


# ---- a tree the user already has ----------------------------------------------------------------------------------------

def table_of_newick(text: str, ids: Sequence[str]):
    """The join table ``(slots int32 [T], lengths float64 [T])``, in the row order of ``ids``, of a Newick tree over exactly
    the names of ``ids``.  A root with two children is one unrooted edge whose lengths add; a missing length is 0.0.
    ``ValueError`` with a one-line reason for text that is no tree, a polytomy (or a node with one child), a different or
    duplicate leaf set and fewer than four leaves."""
    from .bme import Tree, joins_of_tree
    from .treecmp import parse_newick
    n = len(ids)
    index = {str(name): x for x, name in enumerate(ids)}
    if len(index) != n:
        raise ValueError("the alignment's names are not distinct")
    try:
        root = parse_newick(text)
    except RecursionError:
        raise ValueError("the tree is nested too deeply to read") from None
    # (children before parents in reversed(order))
    order = [root]
    for node in order:
        order.extend(node.children)
    names = [node.name for node in order if node.is_leaf()]
    if len(set(names)) != len(names):
        raise ValueError("duplicate leaf names")
    if set(names) != set(index):
        missing, extra = sorted(set(index) - set(names)), sorted(str(x) for x in set(names) - set(index))
        raise ValueError(f"the tree's leaves are not the alignment's sequences ({len(missing)} missing, {len(extra)} unknown"
                         + (f"; first: {(missing or extra)[0]}" if missing or extra else "") + ")")
    if n < MIN_SEQS:
        raise ValueError(f"{FEW_SEQUENCES} ({n})")
    length = {id(node): float(node.length or 0.0) for node in order}
    kids = {id(node): list(node.children) for node in order}
    if len(kids[id(root)]) == 2:
        # one unrooted edge: the inner child becomes the root, the other hangs from it by the sum of the two lengths
        a, b = kids[id(root)]
        top, other = (b, a) if a.is_leaf() else (a, b)
        length[id(other)] = length[id(a)] + length[id(b)]
        kids[id(top)] = kids[id(top)] + [other]
        order = [top] + [node for node in order if node is not root and node is not top]
        root = top
    inner = [node for node in order if kids[id(node)]]
    for node in inner:
        want = 3 if node is root else 2
        if len(kids[id(node)]) != want:
            what = "the root" if node is root else "a node"
            raise ValueError(f"{what} has {len(kids[id(node)])} children: only binary trees (a root of two or three) have a join table")
    assert len(inner) == n - 2
    tree = Tree.__new__(Tree)
    tree.n, tree.root = n, 2 * n - 3
    tree.parent = np.full(2 * n - 2, -1, dtype=np.int32)
    tree.children = np.full((2 * n - 2, 3), -1, dtype=np.int32)
    number = {id(root): tree.root}
    number.update({id(node): n + k for k, node in enumerate(v for v in inner if v is not root)})
    number.update({id(node): index[node.name] for node in order if node.is_leaf()})
    edge = np.zeros(2 * n - 2, dtype=np.float64)
    for node in order:
        edge[number[id(node)]] = 0.0 if node is root else length[id(node)]
        if kids[id(node)]:
            tree._adopt(number[id(node)], [number[id(c)] for c in kids[id(node)]])
    return joins_of_tree(tree, edge)


# ---- the files ----------------------------------------------------------------------------------------------------------

def _num(x) -> str:
    return repr(float(x))


def treedist_tsv(names: Sequence[str], n: int, dist, reasons: Optional[Sequence[Optional[str]]] = None) -> str:
    """``<stem>.treedist.tsv``: one line per pair of ``names`` with ``COLUMNS``; ``dist`` = ``(shared, kf, wrf, ...)`` over
    ``names`` (None: no tree has a table), ``reasons[k]`` says why tree ``k`` has none (it was passed flagged).  A pair
    without a value has ``NA`` and the reasons of its trees in ``note``."""
    reasons = list(reasons) if reasons is not None else [None] * len(names)
    lines = ["\t".join(COLUMNS) + "\n"]
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            s = -1 if dist is None else int(dist[0][i][j])
            if s < 0:
                note = "; ".join(dict.fromkeys(f"{names[k]}: {reasons[k]}" for k in (i, j) if reasons[k])) or "no tree"
                cols = ["NA"] * 4 + [note]
            else:
                rf = rf_of(s, n)
                cols = [str(rf), _num(rf / (2 * (n - 3))), _num(dist[2][i][j]), _num(dist[1][i][j]), ""]
            lines.append("\t".join([str(names[i]), str(names[j])] + cols) + "\n")
    return "".join(lines)


def no_distances(k: int):
    """``join_distances``' results where no tree of ``k`` has a table."""
    return np.full((k, k), -1, dtype=np.int32), np.full((k, k), NAN), np.full((k, k), NAN), 0


def reps_tsv(n: int, dist) -> str:
    """``<stem>.treedist.reps.tsv``: ``dist`` over ``[nj tree, replicate 1 .. R]``; per replicate its ``rf`` and ``kf`` to the
    NJ tree and the mean ``rf`` to the other unflagged replicates (``NA``: flagged, no NJ tree, no other replicate)."""
    shared, kf = dist[0], dist[1]
    K = len(shared)
    lines = ["rep\trf\tkf\tmean_rf\n"]
    for r in range(1, K):
        if int(shared[r][r]) < 0:
            lines.append(f"{r}\tNA\tNA\tNA\n")
            continue
        others = [rf_of(shared[r][q], n) for q in range(1, K) if q != r and int(shared[r][q]) >= 0]
        to_nj = int(shared[0][r]) >= 0
        lines.append("\t".join([str(r), str(rf_of(shared[0][r], n)) if to_nj else "NA", _num(kf[0][r]) if to_nj else "NA",
                                _num(sum(others) / len(others)) if others else "NA"]) + "\n")
    return "".join(lines)


def rf_phylip(n: int, dist) -> str:
    """``<stem>.treedist.rf.phy``: the square RF matrix over ``nj``, ``rep1`` ..., in PHYLIP layout (-1: no value)."""
    shared = dist[0]
    K = len(shared)
    names = ["nj"] + [f"rep{r}" for r in range(1, K)]
    rows = [f"{names[i]:<10}" + " ".join(str(rf_of(shared[i][j], n) if int(shared[i][j]) >= 0 else -1) for j in range(K)) + "\n"
            for i in range(K)]
    return f"{K}\n" + "".join(rows)
