"""Least-squares branch lengths for the ``--ols`` flag of the CLI: the lengths that reproduce the distances best on a FIXED tree.

A tree is a join table in ``Engine.nj_joins``' layout (``fit.py``): only its ``slots int32 [T]`` are read - ordinary least
squares (OLS) depends on the topology alone.  The OLS lengths minimise the residual sum of squares ``--fit`` reports over all
length vectors of that topology; they have a closed form (Rzhetsky & Nei 1993; FastME's ``-w OLS``), an O(N^2) reduction over
the distances.  ``tree_ols_py`` states it; the serial twin (``csrc/pf_ols_host.h``) and the kernels (``csrc/pf_ols.hip.h``) give
its bits.

**Nodes** are ``fit.nodes_of``'s: leaves ``0 .. N-1``; join ``t`` makes node ``N + t`` with children (node in slot ``a``, node in
slot ``b``), in that order; ``R = 2N - 3`` has the last three as children ``c0, c1, c2`` in table order.  ``kids [T]`` names the node
behind every entry of the table; the branch above ``kids[k]`` is written to ``ols[k]``.  ``n(v)`` counts the leaves of ``v``.

**Leaf order.**  ``lo[R] = 0``; children follow each other in child order (``lo[a] = lo[v]``, ``lo[b] = lo[v] + n(a)``; at ``R``,
``c1`` follows ``c0`` and ``c2`` follows ``c1``); ``ord[lo[x]] = x`` for a leaf ``x``; ``sub(v) = ord[lo[v] : lo[v] + n(v)]``.  Sizes are
computed in ascending node order, ``lo`` in descending order: no stack.

**Column sums.**  ``W[y][x] = float64(pred(x, y))`` for leaves ``x != y``, ``W[x][x] = +0.0``; ``W[v][x] = W[a][x] + W[b][x]`` for a join
node; ``r[x] = (W[c0][x] + W[c1][x]) + W[c2][x]``.  The tree fixes the order of these additions.

**Group sum** ``G(X, f)`` over ``x`` in ``sub(X)`` of ``f[x]``, in ``fit.py``'s order: 64 accumulators from ``+0.0``, lane ``l`` takes ``k = l,
l + 64, ... < n(X)`` ascending with ``x = ord[lo[X] + k]``, then ``acc[l] += acc[l + s]`` for ``s = 32, 16, ... 1`` over ``l < s``.

**Per branch** above a non-root node ``v`` with parent ``p``: the upper side is, for ``p == R``, the other two children ``C, D`` of
``R`` in table order with ``f_D = W[D]``, ``nD = n(D)``; else ``C`` is ``v``'s sibling, ``f_D[x] = r[x] - W[p][x]`` and ``nD = N - n(p)``.
Averages are ``d_XY = S_XY / (float64(nX) float64(nY))``; ``S_CD = G(C, f_D)``.  A leaf: ``l = 0.5 ((W[C][v] / nC + f_D[v] / nD) -
d_CD)``.  A join node ``v = (a, b)``: ``S_AB = G(a, W[b])``, ``S_AC = G(a, W[C])``, ``S_BC = G(b, W[C])``, ``S_AD = G(a, f_D)``, ``S_BD = G(b,
f_D)``, ``gamma = (nB nC + nA nD) / ((nA + nB) (nC + nD))`` and ``l = 0.5 ((gamma (d_AC + d_BD) + (1 - gamma) (d_BC + d_AD)) - (d_AB +
d_CD))``.  Every product, quotient and sum is rounded where it is written.

**Status per tree.**  0 fine; 2 the table is no join table (``fit.table_status``, checked first); 1 a NaN or an infinity among the
distances.  Any status but 0: zeros.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence, Tuple

import numpy as np

from .fit import (LANES, MAX_SEQS, MIN_SEQS, NO_TABLE, NONFINITE, OK, n_of_pairs, pair_index, table_len, table_status)
from .treearrays import unbatched

# From that many sequences on, a kind whose table is made on the GPU thread has its OLS lengths computed there (Engine.tree_ols
# and one Engine.tree_fit of both tables); below, the writer thread's host side calls the twin.  A measured constant, the
# smallest size of tools/ols_bench.py from which the device is ahead for all three tables (profiles/ols_bench.txt):
# Engine.tree_ols of ONE tree, staging included, takes 0.08 ms at 20, 0.10 ms at 60 and 0.23 ms at 200 sequences against the
# twin's 0.01 - 0.04, 0.03 - 0.04 and 0.11 (balanced), 0.12 (NJ), 0.21 ms (caterpillar); at 512 it takes 0.52 ms against 3.9 -
# 4.1 ms, and from there on it is ahead for every table.  None switches the device route off.
OLS_DEVICE_MIN = 512


def refuse(b: int, m: int, n: int):
    """What the three entry points refuse, with their messages."""
    if n < MIN_SEQS:
        raise ValueError(f"tree OLS needs N >= {MIN_SEQS} sequences (got {n})")
    if n > MAX_SEQS:
        raise ValueError(f"tree OLS takes at most {MAX_SEQS} sequences (got {n})")
    if b < 1:
        raise ValueError(f"tree OLS needs B >= 1 sources (got {b})")
    if m < 1:
        raise ValueError(f"tree OLS needs M >= 1 trees per source (got {m})")


def ols_arrays(preds, slots):
    """The arguments of the three ``pf_tree_ols`` entry points, checked, in ``fit.fit_arrays``' shapes: ``preds`` is ``[B, P_N]``
    with tables ``[B, M, T]`` (or ``[B, T]``: the results come without ``M``) or ``[P_N]`` with tables ``[M, T]`` (or ``[T]``).  →
    ``(preds float32 [B, P_N], slots int32 [B, M, T], (B, M, N), (single, one), zeroed (ols, status))``."""
    p = np.ascontiguousarray(np.asarray(preds, dtype=np.float32))
    s = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
    single = p.ndim == 1
    if single:
        p, s = p[None], s[None]
    one = s.ndim == 2
    if one:
        s = s[:, None, :]
    if p.ndim != 2 or s.ndim != 3 or s.shape[0] != p.shape[0]:
        raise ValueError(f"expected distances [B, P] and tables [B, M, T], got {np.shape(preds)} and {np.shape(slots)}")
    n = n_of_pairs(p.shape[1])
    b, m, t = s.shape
    if n * (n - 1) // 2 != p.shape[1] or (n >= 3 and t != table_len(n)):
        raise ValueError(f"{p.shape[1]} distances and {t} slots are not those of one number of sequences")
    refuse(b, m, n)
    return p, s, (b, m, n), (single, one), (np.zeros((b, m, t), dtype=np.float64), np.zeros((b, m), dtype=np.uint8))


def squeezed(out, flags):
    """The results without ``M`` and ``B`` where the arguments came without them."""
    single, one = flags
    if one:
        out = tuple(x[:, 0] for x in out)
    return unbatched(out, single)


# ---- the statement ------------------------------------------------------------------------------------------------------

def kids_of(slots: Sequence[int], n: int) -> np.ndarray:
    """``kids int32 [T]`` of a join table (status 0): the node behind every entry - the children of node ``n + t`` at ``2t`` and
    ``2t + 1``, those of the last node at ``2 (n - 3) + k``."""
    kids = np.zeros(table_len(n), dtype=np.int32)
    node = list(range(n))
    for t in range(n - 3):
        a, b = int(slots[2 * t]), int(slots[2 * t + 1])
        kids[2 * t], kids[2 * t + 1] = node[a], node[b]
        node[a] = n + t
    for k in range(3):
        kids[2 * (n - 3) + k] = node[int(slots[2 * (n - 3) + k])]
    return kids


def leaf_order(kids: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(count int32 [2n - 2], lo int32 [2n - 2], ord int32 [n])``: sizes in ascending node order, ``lo`` in descending."""
    joins, root = n - 3, 2 * n - 3
    count, lo = np.ones(2 * n - 2, dtype=np.int32), np.zeros(2 * n - 2, dtype=np.int32)
    for t in range(joins):
        count[n + t] = count[kids[2 * t]] + count[kids[2 * t + 1]]
    c0, c1, c2 = (int(kids[2 * joins + k]) for k in range(3))
    count[root] = n
    lo[c0], lo[c1], lo[c2] = 0, count[c0], count[c0] + count[c1]
    for t in range(joins - 1, -1, -1):
        a, b = int(kids[2 * t]), int(kids[2 * t + 1])
        lo[a], lo[b] = lo[n + t], lo[n + t] + count[a]
    order = np.zeros(n, dtype=np.int32)
    order[lo[:n]] = np.arange(n, dtype=np.int32)
    return count, lo, order


def column_sums(pred: np.ndarray, kids: np.ndarray, n: int) -> np.ndarray:
    """``W float64 [2n - 2, n]``: the rows of the leaves, of the join nodes in their order, and ``r`` as the last node's.  (A row
    is added as a whole here: the additions of one column are those of the text, and no column meets another.)"""
    w = np.zeros((2 * n - 2, n), dtype=np.float64)
    d = np.asarray(pred, dtype=np.float32).astype(np.float64)
    for x in range(n):
        for y in range(x + 1, n):
            w[y, x] = w[x, y] = d[pair_index(x, y, n)]
    joins = n - 3
    for t in range(joins):
        w[n + t] = w[kids[2 * t]] + w[kids[2 * t + 1]]
    w[2 * n - 3] = (w[kids[2 * joins]] + w[kids[2 * joins + 1]]) + w[kids[2 * joins + 2]]
    return w


def group_sum(f: np.ndarray) -> float:
    """``G`` of the values ``f[ord[lo[X] + k]]``, given in the order of ``k``: 64 strided accumulators, then the pairwise
    combination.  (The tail is padded with ``+0.0``: an accumulator that started from ``+0.0`` is never ``-0.0``, so adding
    ``+0.0`` to it changes no bit.)"""
    rows = -(-len(f) // LANES)
    padded = np.zeros(max(rows, 1) * LANES, dtype=np.float64)
    padded[:len(f)] = f
    acc = np.zeros(LANES, dtype=np.float64)
    for row in padded.reshape(-1, LANES):
        acc = acc + row
    s = LANES // 2
    while s:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return float(acc[0])


def tree_ols_py(pred, slots, n: int):
    """The statement, one source's distances ``pred float32 [P_n]`` and ONE join table's ``slots int32 [T]``: ``(ols float64 [T],
    status uint8 scalar)``."""
    pred, slots = np.asarray(pred, dtype=np.float32), np.asarray(slots, dtype=np.int32)
    refuse(1, 1, n)
    pairs, width = n * (n - 1) // 2, table_len(n)
    if pred.shape != (pairs,) or slots.shape != (width,):
        raise ValueError(f"expected {pairs} distances and {width} slots for {n} sequences, got {pred.shape} and {slots.shape}")
    ols = np.zeros(width, dtype=np.float64)
    if table_status(slots, n) != OK:
        return ols, np.uint8(NO_TABLE)
    if not np.isfinite(pred).all():
        return ols, np.uint8(NONFINITE)
    kids = kids_of(slots, n)
    count, lo, order = leaf_order(kids, n)
    w = column_sums(pred, kids, n)
    joins, root = n - 3, 2 * n - 3
    f64 = np.float64

    def sub(v):
        return order[lo[v]:lo[v] + count[v]]

    def mean(s, nx, ny):
        return f64(s) / (f64(nx) * f64(ny))

    with np.errstate(all="ignore"):
        for k in range(width):
            v = int(kids[k])
            if k < 2 * joins:
                p, c = n + k // 2, int(kids[k ^ 1])
                f_d, n_d = w[root] - w[p], n - int(count[p])
            else:
                c, d = (int(kids[2 * joins + i]) for i in range(3) if 2 * joins + i != k)
                f_d, n_d = w[d], int(count[d])
            n_c = int(count[c])
            d_cd = mean(group_sum(f_d[sub(c)]), n_c, n_d)
            if v < n:
                ols[k] = f64(0.5) * ((w[c, v] / f64(n_c) + f_d[v] / f64(n_d)) - d_cd)
                continue
            a, b = int(kids[2 * (v - n)]), int(kids[2 * (v - n) + 1])
            n_a, n_b = int(count[a]), int(count[b])
            d_ab = mean(group_sum(w[b][sub(a)]), n_a, n_b)
            d_ac = mean(group_sum(w[c][sub(a)]), n_a, n_c)
            d_bc = mean(group_sum(w[c][sub(b)]), n_b, n_c)
            d_ad = mean(group_sum(f_d[sub(a)]), n_a, n_d)
            d_bd = mean(group_sum(f_d[sub(b)]), n_b, n_d)
            gamma = (f64(n_b) * f64(n_c) + f64(n_a) * f64(n_d)) / ((f64(n_a) + f64(n_b)) * (f64(n_c) + f64(n_d)))
            ols[k] = f64(0.5) * ((gamma * (d_ac + d_bd) + (f64(1.0) - gamma) * (d_bc + d_ad)) - (d_ab + d_cd))
    return ols, np.uint8(OK)


def tree_ols_batch_py(preds, slots):
    """``tree_ols_py`` of every tree of every source, with ``Engine.tree_ols``' arguments and results: the host side of
    ``--python-io`` (``treekinds.PythonHost``)."""
    p, s, (b, m, n), flags, out = ols_arrays(preds, slots)
    for k in range(b):
        for r in range(m):
            out[0][k, r], out[1][k, r] = tree_ols_py(p[k], s[k, r], n)
    return squeezed(out, flags)


# ---- derived in Python only ---------------------------------------------------------------------------------------------

class Scores(NamedTuple):
    """What ``--ols`` reports of one tree, from the unclamped tables; ``nan`` for a tree with a status."""
    length: float            # the tree length: the sum of the table's own branch lengths, in table order
    length_ols: float        # that of the OLS lengths
    rmse: float              # fit.Scores.rmse of the table's own lengths
    rmse_ols: float
    explained: float         # fit.Scores.explained
    explained_ols: float
    negative: int            # branches below zero among the table's own lengths
    negative_ols: int
    most_negative_ols: float     # the smallest OLS length where one is negative, else 0
    max_change: float        # max |ols - lengths|


def tree_length(lengths) -> float:
    """The sum of the branch lengths, added in table order."""
    total = 0.0
    for x in np.asarray(lengths, dtype=np.float64).tolist():
        total = total + x
    return total


def ols_scores(pred, lengths, ols, rows, worst_j, n: int) -> Scores:
    """The derived figures of one tree (status 0): its own ``lengths [T]``, the OLS ``ols [T]`` and ``tree_fit``'s ``rows [2, n, 6]`` /
    ``worst_j [2, n]`` of the two tables ``[lengths, ols]`` stacked on the same slots."""
    from .fit import fit_scores
    lengths, ols = np.asarray(lengths, dtype=np.float64), np.asarray(ols, dtype=np.float64)
    own, best = fit_scores(pred, rows[0], worst_j[0], n), fit_scores(pred, rows[1], worst_j[1], n)
    return Scores(tree_length(lengths), tree_length(ols), own.rmse, best.rmse, own.explained, best.explained,
                  int((lengths < 0).sum()), int((ols < 0).sum()), min(float(ols.min()), 0.0), float(np.abs(ols - lengths).max()))


def no_scores() -> Scores:
    """The scores of a tree with a status (distances that are not finite) or of fewer than three sequences."""
    nan = float("nan")
    return Scores(nan, nan, nan, nan, nan, nan, 0, 0, nan, nan)


# ---- the file of --ols --------------------------------------------------------------------------------------------------

OLS_HEAD = ("kind\tlength\tlength_ols\trmse\trmse_ols\texplained\texplained_ols\tnegative\tnegative_ols\tmost_negative_ols\t"
            "max_change\n")


def ols_line(kind: str, s: Scores) -> str:
    """One kind's line of ``<stem>.ols.tsv``."""
    return (f"{kind}\t{s.length:.10g}\t{s.length_ols:.10g}\t{s.rmse:.10g}\t{s.rmse_ols:.10g}\t{s.explained:.10f}\t"
            f"{s.explained_ols:.10f}\t{s.negative}\t{s.negative_ols}\t{s.most_negative_ols:.10g}\t{s.max_change:.10g}\n")


def ols_tsv(lines: Sequence[Tuple[str, Scores]]) -> str:
    """``<stem>.ols.tsv``: one line per written kind."""
    return OLS_HEAD + "".join(ols_line(kind, s) for kind, s in lines)


def parse_ols_tsv(text: str) -> dict:
    """``{kind: Scores}`` of a ``<stem>.ols.tsv``."""
    out = {}
    for row in text.splitlines()[1:]:
        c = row.split("\t")
        out[c[0]] = Scores(*(int(x) if k in (6, 7) else float(x) for k, x in enumerate(c[1:])))
    return out
