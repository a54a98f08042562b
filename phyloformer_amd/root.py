"""Tree rooting for the ``--root`` flag of the CLI: where the root of an unrooted tree is, by minimal ancestor deviation (MAD;
Tria, Landan & Dagan 2017, Nat. Ecol. Evol. 1:0193) and by the midpoint of the longest path.

A tree is a join table in ``Engine.nj_joins``' layout (``fit.py``): ``slots int32 [T]`` and ``lengths float64 [T]``.  No distances
are read.  ``tree_root_py`` states the computation; the serial twin (``csrc/pf_root_host.h``) and the kernels
(``csrc/pf_root.hip.h``) give its bits.  Every product, quotient and sum is rounded where it is written.

**Nodes, leaf order, lengths.**  Nodes are ``fit.nodes_of``'s; ``kids``, ``count``, ``lo`` and ``ord`` are ``ols.kids_of`` and
``ols.leaf_order``.  ``pos[x] = lo[x]`` is the place of leaf ``x`` in ``ord``; leaf ``x`` is *below* node ``v`` iff ``lo[v] <= pos[x] <
lo[v] + n(v)``.  Lengths are clamped for the whole computation: ``L(v) = max(length above v, +0.0)``.

**Node-to-leaf path lengths** ``D float64 [2N-2][N]``, one column ``x`` at a time, no column reading another: ``D[x][x] = +0.0``;
ascending over the join nodes ``v`` and then ``R``, for the child ``c`` with ``x`` below it ``D[v][x] = D[c][x] + L(c)``; descending from
``v = 2N-4`` to ``0`` with parent ``p``, if ``x`` is not below ``v``, ``D[v][x] = D[p][x] + L(v)``.

**Weights.**  ``W[b][c] = 1.0 / (D[b][c] * D[b][c])`` where ``D[b][c] > 0``, else ``+0.0``.

**Per entry** ``k`` (node ``v = kids[k]``, the branch above it, a root at ``lam`` above ``v``), all in tree leaf order ``q = pos[x]``:
*position* - for ``q`` in ``v``'s range and ``c`` outside it, ascending ``c``, one sequential accumulator each from ``+0.0``: ``r1[q] = sum
W[q][c] * (D[v][q] - D[v][c])``, ``r0[q] = sum W[q][c]``; ``S1``, ``S0`` their group sums over ``sub(v)`` in ``ols.group_sum``'s order; ``lam =
0`` if ``S0 == 0`` else ``min(max(-S1 / (2 S0), 0), L(v))``.  *Score* - ``t[q] = D[v][q] + lam`` in the range, ``D[v][q] - lam`` outside; for every
``q`` over all ``c`` ascending ``r[q] = sum W[q][c] * ((t[q] - t[c]) * (t[q] - t[c]))``; ``ssq[k] = 0.5 * G(all q ascending, r)``.

**Midpoint.**  The pair ``b < c`` with the largest ``D[c][b]``, first in pair order; ``half = 0.5 * D[c][b]``; the first entry ``k`` in table
order whose node separates ``b`` and ``c`` with ``lo <= half <= hi``, ``(lo, hi) = (D[v][b], D[p][b])`` if ``b`` is below ``v``, ``(D[p][b], D[v][b])``
if ``c`` is; ``lam_mid = half - D[v][b]`` or ``D[v][b] - half``.  ``mid = (k, lam_mid, b, c, D[c][b])``.

**Status per tree.**  0 fine; 2 no join table (``fit.table_status``, checked first); 1 a NaN or an infinity among the lengths.  Any
status but 0: zeros.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Sequence, Tuple

import numpy as np

from .fit import MAX_SEQS, MIN_SEQS, NO_TABLE, NONFINITE, OK, nodes_of, table_len, table_status
from .ols import group_sum, kids_of, leaf_order
from .treearrays import unbatched

MID = 5          # mid: k, lam_mid, b, c, D[c][b]
# From that many sequences on, a kind whose table is made on the GPU thread is rooted there (Engine.tree_root); below, the
# writer thread's host side calls the twin.  A measured constant, the smallest size of tools/root_bench.py from which the device
# is ahead for all three tables (profiles/root_bench.txt): Engine.tree_root of ONE tree, staging included, takes 0.15 ms at 20
# sequences against the twin's 0.04 - 0.07, 0.21 ms at 60 against 0.23 (balanced), 0.26 (NJ) and 0.30 ms (caterpillar), 0.40 -
# 0.42 ms at 200 against 8.4 - 9.2 ms, and from there on the twin's O(N^3) leaves it behind (1.2 ms against 0.47 - 0.51 s at
# 512).  Just below NJ's own device threshold, at 255 sequences, the host route costs 17.5 - 19.5 ms a tree.  None switches the
# device route off.
ROOT_DEVICE_MIN = 60
METHODS = ("mad", "midpoint")


def refuse(b: int, m: int, n: int):
    """What the three entry points refuse, with their messages."""
    if n < MIN_SEQS:
        raise ValueError(f"tree root needs N >= {MIN_SEQS} sequences (got {n})")
    if n > MAX_SEQS:
        raise ValueError(f"tree root takes at most {MAX_SEQS} sequences (got {n})")
    if b < 1:
        raise ValueError(f"tree root needs B >= 1 sources (got {b})")
    if m < 1:
        raise ValueError(f"tree root needs M >= 1 trees per source (got {m})")


def root_arrays(slots, lengths):
    """The arguments of the three ``pf_tree_root`` entry points, checked, in ``ols.ols_arrays``' shapes: tables ``[B, M, T]``, ``[B, T]``
    (the results come without ``M``) or ``[T]`` (without ``B`` too).  → ``(slots int32 [B, M, T], lengths float64 [B, M, T], (B, M, N),
    (single, one), zeroed (ssq, pos, mid, status))``."""
    s = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
    l = np.ascontiguousarray(np.asarray(lengths, dtype=np.float64))
    if s.shape != l.shape or not 1 <= s.ndim <= 3:
        raise ValueError(f"expected slots and lengths [B, M, T], [B, T] or [T], got {np.shape(slots)} and {np.shape(lengths)}")
    single = s.ndim == 1
    if single:
        s, l = s[None], l[None]
    one = s.ndim == 2
    if one:
        s, l = s[:, None, :], l[:, None, :]
    b, m, t = s.shape
    n = (t + 3) // 2
    if t < 1 or t % 2 == 0:
        raise ValueError(f"{t} slots are the table of no number of sequences")
    refuse(b, m, n)
    out = (np.zeros((b, m, t), dtype=np.float64), np.zeros((b, m, t), dtype=np.float64), np.zeros((b, m, MID), dtype=np.float64),
           np.zeros((b, m), dtype=np.uint8))
    return s, l, (b, m, n), (single, one), out


def squeezed(out, flags):
    """The results without ``M`` and ``B`` where the arguments came without them."""
    single, one = flags
    if one:
        out = tuple(x[:, 0] for x in out)
    return unbatched(out, single)


# ---- the statement ------------------------------------------------------------------------------------------------------

def clamped_nodes(slots, lengths, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(parent int32 [2n - 2], L float64 [2n - 2])``: ``fit.nodes_of`` with every length clamped at ``+0.0``."""
    parent, blen = nodes_of(slots, lengths, n)
    return parent, np.where(blen > 0.0, blen, 0.0)


def path_lengths(parent: np.ndarray, blen: np.ndarray, count: np.ndarray, lo: np.ndarray, n: int) -> np.ndarray:
    """``D float64 [2n - 2, n]`` with the columns in leaf order: ``D[v][pos[x]]`` is the path from node ``v`` to leaf ``x``.  (A row is
    filled as a whole: the additions of one column are those of the text.)"""
    nodes, root = 2 * n - 2, 2 * n - 3
    q = np.arange(n)
    below = (lo[:, None] <= q[None, :]) & (q[None, :] < (lo + count)[:, None])
    d = np.zeros((nodes, n), dtype=np.float64)
    for v in range(root):            # ascending: a child is visited before its parent
        p = int(parent[v])
        d[p] = np.where(below[v], d[v] + blen[v], d[p])
    for v in range(root - 1, -1, -1):
        d[v] = np.where(below[v], d[v], d[int(parent[v])] + blen[v])
    return d


def weights(d: np.ndarray, order: np.ndarray, n: int) -> np.ndarray:
    """``W float64 [n, n]`` in leaf order on both sides: ``W[q][c]`` of the leaves ``ord[q]`` and ``ord[c]``."""
    leaf = d[order]
    with np.errstate(all="ignore"):
        return np.where(leaf > 0.0, 1.0 / (leaf * leaf), 0.0)


def position(s1: float, s0: float, length: float) -> float:
    """``min(max(-S1 / (2 S0), +0.0), L)``, ``+0.0`` where ``S0 == 0``; a zero is ``+0.0``."""
    if s0 == 0.0:
        return 0.0
    x = -s1 / (2.0 * s0)
    x = x if x > 0.0 else 0.0
    return x if x < length else length


def midpoint(d, kids, parent, count, lo, n: int) -> np.ndarray:
    """``mid float64 [5]`` of the text."""
    best, pair = -1.0, (0, 1)
    for b in range(n - 1):
        col = d[b + 1:n, lo[b]]
        c = int(np.argmax(col))
        if col[c] > best:
            best, pair = float(col[c]), (b, b + 1 + c)
    b, c = pair
    half = 0.5 * best

    def below(v, x):
        return lo[v] <= lo[x] < lo[v] + count[v]

    for k, v in enumerate(kids.tolist()):
        p = int(parent[v])
        if below(v, b) and not below(v, c) and d[v, lo[b]] <= half <= d[p, lo[b]]:
            return np.array([k, half - d[v, lo[b]], b, c, best], dtype=np.float64)
        if below(v, c) and not below(v, b) and d[p, lo[b]] <= half <= d[v, lo[b]]:
            return np.array([k, d[v, lo[b]] - half, b, c, best], dtype=np.float64)
    raise AssertionError("column b tiles the path: a branch holds the midpoint")


def tree_root_py(slots, lengths, n: int):
    """The statement, ONE join table: ``(ssq float64 [T], pos float64 [T], mid float64 [5], status uint8 scalar)``."""
    slots, lengths = np.asarray(slots, dtype=np.int32), np.asarray(lengths, dtype=np.float64)
    refuse(1, 1, n)
    width = table_len(n)
    if slots.shape != (width,) or lengths.shape != (width,):
        raise ValueError(f"expected {width} slots and lengths for {n} sequences, got {slots.shape} and {lengths.shape}")
    ssq, pos, mid = np.zeros(width, dtype=np.float64), np.zeros(width, dtype=np.float64), np.zeros(MID, dtype=np.float64)
    if table_status(slots, n) != OK:
        return ssq, pos, mid, np.uint8(NO_TABLE)
    if not np.isfinite(lengths).all():
        return ssq, pos, mid, np.uint8(NONFINITE)
    kids = kids_of(slots, n)
    count, lo, order = leaf_order(kids, n)
    parent, blen = clamped_nodes(slots, lengths, n)
    d = path_lengths(parent, blen, count, lo, n)
    w = weights(d, order, n)
    q = np.arange(n)
    dv = d[kids]                                                         # [T, n]: row k is D[v_k]
    inside = (lo[kids][:, None] <= q[None, :]) & (q[None, :] < (lo[kids] + count[kids])[:, None])
    # position: per (k, q in the range) the sums over c outside it, ascending c
    r1, r0 = np.zeros((width, n), dtype=np.float64), np.zeros((width, n), dtype=np.float64)
    for c in range(n):
        take = inside & ~inside[:, c:c + 1]
        r1 = np.where(take, r1 + w[None, :, c] * (dv - dv[:, c:c + 1]), r1)
        r0 = np.where(take, r0 + w[None, :, c], r0)
    for k in range(width):
        v = int(kids[k])
        s1, s0 = group_sum(r1[k, lo[v]:lo[v] + count[v]]), group_sum(r0[k, lo[v]:lo[v] + count[v]])
        pos[k] = position(s1, s0, float(blen[v]))
    # score: per (k, q) the sum over all c ascending
    t = np.where(inside, dv + pos[:, None], dv - pos[:, None])
    r = np.zeros((width, n), dtype=np.float64)
    for c in range(n):
        diff = t - t[:, c:c + 1]
        r = r + w[None, :, c] * (diff * diff)
    for k in range(width):
        ssq[k] = 0.5 * group_sum(r[k])
    return ssq, pos, midpoint(d, kids, parent, count, lo, n), np.uint8(OK)


def tree_root_batch_py(slots, lengths):
    """``tree_root_py`` of every tree, with ``Engine.tree_root``'s arguments and results: the host side of ``--python-io``."""
    s, l, (b, m, n), flags, out = root_arrays(slots, lengths)
    for k in range(b):
        for r in range(m):
            out[0][k, r], out[1][k, r], out[2][k, r], out[3][k, r] = tree_root_py(s[k, r], l[k, r], n)
    return squeezed(out, flags)


# ---- derived in Python only ---------------------------------------------------------------------------------------------

class Scores(NamedTuple):
    """What ``--root`` reports of one tree; ``nan`` for a tree with a status."""
    mad: float               # sqrt(ssq / P_N) of the MAD root branch, the first minimum of ssq
    ambiguity: float         # that over the second smallest (Tria's AI), in (0, 1]; 1 where both are 0
    root_k: int              # the entry of the table whose branch holds the MAD root
    root_below: int          # leaves below that branch
    root_pos: float          # the root's distance above the branch's lower node
    root_length: float       # the branch's clamped length
    clock_cv: float          # the coefficient of variation of the root-to-tip distances (Tria's root clock CV)
    mid_i: int
    mid_j: int
    mid_diameter: float
    mid_k: int
    mid_below: int
    mid_pos: float
    mid_clock_cv: float
    same_branch: bool


def tip_distances(slots, lengths, k: int, lam: float, n: int) -> np.ndarray:
    """The root-to-tip distances ``float64 [n]``, by sequence, of a root ``lam`` above the node of entry ``k``."""
    kids = kids_of(slots, n)
    count, lo, _order = leaf_order(kids, n)
    parent, blen = clamped_nodes(slots, lengths, n)
    d = path_lengths(parent, blen, count, lo, n)
    v = int(kids[k])
    inside = (lo[v] <= lo[:n]) & (lo[:n] < lo[v] + count[v])
    row = d[v][lo[:n]]
    return np.where(inside, row + lam, row - lam)


def clock_cv(tips: np.ndarray) -> float:
    mean = float(np.mean(tips))
    return float(np.std(tips)) / mean if mean > 0.0 else 0.0


def root_scores(slots, lengths, ssq, pos, mid, n: int) -> Scores:
    """The derived figures of one tree (status 0)."""
    ssq, pos = np.asarray(ssq, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    kids = kids_of(slots, n)
    count, _lo, _order = leaf_order(kids, n)
    _parent, blen = clamped_nodes(slots, lengths, n)
    k = int(np.argmin(ssq))
    mads = np.sqrt(ssq / (n * (n - 1) // 2))
    two = np.sort(mads)[:2]
    ambiguity = 1.0 if two[1] == 0.0 else float(two[0] / two[1])
    mk = int(mid[0])
    return Scores(float(mads[k]), ambiguity, k, int(count[kids[k]]), float(pos[k]), float(blen[kids[k]]),
                  clock_cv(tip_distances(slots, lengths, k, float(pos[k]), n)), int(mid[2]), int(mid[3]), float(mid[4]), mk,
                  int(count[kids[mk]]), float(mid[1]), clock_cv(tip_distances(slots, lengths, mk, float(mid[1]), n)), k == mk)


def no_scores() -> Scores:
    """The scores of a tree with a status or of fewer than three sequences."""
    nan = float("nan")
    return Scores(nan, nan, -1, 0, nan, nan, nan, -1, -1, nan, -1, 0, nan, nan, False)


def root_choice(scores: Scores, method: str) -> Tuple[int, float]:
    """``(k, lam)`` of the method's root."""
    if method not in METHODS:
        raise ValueError(f"--root takes one of {', '.join(METHODS)} (got {method})")
    return (scores.root_k, scores.root_pos) if method == "mad" else (scores.mid_k, scores.mid_pos)


def rooted_newick(ids: Sequence[str], slots, lengths, k: int, lam: float, clamp_negative: bool = True) -> str:
    """The text of the join table rooted ``lam`` above the node of entry ``k``: the root has two children, the subtree below that node
    by ``lam`` and the rest by ``L - lam``; every other branch is formatted and clamped as ``nj.newick_of_joins`` does it."""
    n = len(ids)
    slots, lengths = np.asarray(slots, dtype=np.int32), np.asarray(lengths, dtype=np.float64)
    kids = kids_of(slots, n)
    parent, own = nodes_of(slots, lengths, n)
    joins, root = n - 3, 2 * n - 3

    def fmt(x: float) -> str:
        if clamp_negative and x < 0:
            x = 0.0
        return repr(float(x))

    down = [str(i) for i in ids] + [""] * (joins + 1)
    for t in range(joins):
        a, b = int(kids[2 * t]), int(kids[2 * t + 1])
        down[n + t] = f"({down[a]}:{fmt(own[a])},{down[b]}:{fmt(own[b])})"
    v = int(kids[k])
    full = max(float(own[v]), 0.0)
    head, tail, u = [], [], v
    while int(parent[u]) != root:
        p = int(parent[u])
        a, b = int(kids[2 * (p - n)]), int(kids[2 * (p - n) + 1])
        sib = b if a == u else a
        head.append(f"({down[sib]}:{fmt(own[sib])},")
        tail.append(f":{fmt(own[p])})")
        u = p
    others = [int(c) for c in kids[2 * joins:] if int(c) != u]
    rest = "".join(head) + "(" + ",".join(f"{down[c]}:{fmt(own[c])}" for c in others) + ")" + "".join(reversed(tail))
    return f"({down[v]}:{fmt(lam)},{rest}:{fmt(full - lam)});\n"


# ---- the file of --root -------------------------------------------------------------------------------------------------

ROOT_HEAD = ("kind\tmethod\tmad\tambiguity\troot_below\troot_pos\troot_length\tclock_cv\tmid_i\tmid_j\tmid_diameter\tmid_below\t"
             "mid_pos\tmid_clock_cv\tsame_branch\n")


def root_line(kind: str, method: str, s: Scores, ids: Sequence[str] = ()) -> str:
    """One kind's line of ``<stem>.root.tsv``; the midpoint pair by name where ``ids`` are given."""
    def name(i):
        return ids[i] if ids and i >= 0 else str(i)
    same = "nan" if math.isnan(s.mad) else str(int(s.same_branch))
    return (f"{kind}\t{method}\t{s.mad:.10g}\t{s.ambiguity:.10g}\t{s.root_below}\t{s.root_pos:.10g}\t{s.root_length:.10g}\t"
            f"{s.clock_cv:.10g}\t{name(s.mid_i)}\t{name(s.mid_j)}\t{s.mid_diameter:.10g}\t{s.mid_below}\t{s.mid_pos:.10g}\t"
            f"{s.mid_clock_cv:.10g}\t{same}\n")


def root_tsv(lines) -> str:
    """``<stem>.root.tsv``: one line per written kind, ``lines`` of ``(kind, method, Scores, ids)``."""
    return ROOT_HEAD + "".join(root_line(*line) for line in lines)


def parse_root_tsv(text: str) -> dict:
    """``{kind: {column: text}}`` of a ``<stem>.root.tsv``."""
    head = ROOT_HEAD.rstrip("\n").split("\t")
    return {row.split("\t")[0]: dict(zip(head, row.split("\t"))) for row in text.splitlines()[1:]}
