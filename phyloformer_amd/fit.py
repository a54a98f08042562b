"""Tree fit for the ``--fit`` flag of the CLI: how well a tree reproduces the distances it was built from.

A tree here is a join table in ``Engine.nj_joins``' layout, whichever kind made it (``treekinds.KINDS``): ``slots int32
[T]`` and ``lengths float64 [T]``, ``T = 2 (N - 3) + 3`` - ``a, b`` / ``la, lb`` per join, slot ``a`` standing for the new
node afterwards, then the last three slots.  Lengths are taken as the table holds them: a negative NJ length is not clamped.

**Nodes.**  Leaves are ``0 .. N-1``; join ``t`` makes node ``N + t`` over the nodes then in slots ``a`` and ``b``; node ``2N - 3``
is the parent of the last three.  A parent's number is above its children's.

**Patristic distance.**  ``T[x, y] = up(x) + up(y)``: ``up(x)`` is the float64 sum of the branch lengths from ``x`` upward to,
but not beyond, the lowest common node, added one after the other from ``+0.0`` in walking order.  There are no products.
``patristic_py`` replays the table with a member list and a height per leaf - ``T[x, y] = (h[x] + la) + (h[y] + lb)`` at the join
that unites them - which is the same sequence of additions.

**Residual and row sums.**  ``e = float64(pred) - T``.  Per sequence ``i`` over ``j != i``: ``ss = sum e e``, ``fm = sum (e e) /
(d d)`` (the Fitch-Margoliash weights; the term is 0 where ``d <= 0``), ``st = sum T``, ``stt = sum T T``, ``sdt = sum d T``, ``worst =
max |e|`` and ``worst_j``, its ``j``, ties to the smallest.  The ORDER is part of the definition: 64 strided accumulators - lane
``l`` takes ``j = l, l + 64, ...`` ascending, skips ``i`` and adds ``acc = acc + term`` from ``+0.0``, every product and quotient
rounded before it is added - then ``for s in 32, 16, 8, 4, 2, 1: acc[l] += acc[l + s]`` for ``l < s``.  One wave per row follows
that order on the device (``csrc/pf_fit.hip.h``), the serial twin follows it on the host (``csrc/pf_fit_host.h``), and all three
agree bit for bit.

**Status per tree.**  0 fine; 1 a NaN or an infinity in the source's distances or the tree's lengths; 2 the table is no join
table (a slot outside ``0 .. N-1``, a slot joined after it left, ``a == b``; checked first).  Any status but 0: zeros everywhere.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Sequence, Tuple

import numpy as np

from .treearrays import unbatched

MIN_SEQS, MAX_SEQS = 3, 8192          # the cap of the three entry points (csrc/pf_fit_host.h)
LANES = 64
COLS = 6                              # ss, fm, st, stt, sdt, worst
SS, FM, ST, STT, SDT, WORST = range(COLS)
OK, NONFINITE, NO_TABLE = 0, 1, 2
# From that many sequences on, a kind whose table is made on the GPU thread has its fit computed there (Engine.tree_fit);
# below, the writer thread's host side calls the twin.  A measured constant (profiles/fit_bench.txt): Engine.tree_fit of ONE
# tree - a launch of one file, the least the GPU thread may hold - takes 0.13 ms at 20 and 0.14 - 0.15 ms at 60 sequences
# against the twin's 0.02 - 0.08 ms, and 0.20 - 0.21 ms at 200 against 0.31 (balanced), 1.65 (caterpillar) and 3.16 ms (NJ);
# from there on it is ahead for every table.  None switches the device path off.
FIT_DEVICE_MIN = 200


def table_len(n: int) -> int:
    return 2 * (n - 3) + 3


def n_of_pairs(pairs: int) -> int:
    """The number of sequences with ``pairs`` pairs; 0 if there is none."""
    n = (1 + int(round((1 + 8 * pairs) ** 0.5))) // 2
    return n if n * (n - 1) // 2 == pairs else 0


def pair_index(i: int, j: int, n: int) -> int:
    """The index of the pair ``i < j`` of ``n`` sequences."""
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def refuse(b: int, m: int, n: int):
    """What the three entry points refuse, with their messages."""
    if n < MIN_SEQS:
        raise ValueError(f"tree fit needs N >= {MIN_SEQS} sequences (got {n})")
    if n > MAX_SEQS:
        raise ValueError(f"tree fit takes at most {MAX_SEQS} sequences (got {n})")
    if b < 1:
        raise ValueError(f"tree fit needs B >= 1 sources (got {b})")
    if m < 1:
        raise ValueError(f"tree fit needs M >= 1 trees per source (got {m})")
    if n * (n - 1) // 2 >= 1 << 31:
        raise ValueError(f"N={n} sequences have 2^31 pairs or more")


def fit_arrays(preds, slots, lengths, patristic: bool = True):
    """The arguments of the three ``pf_tree_fit`` entry points, checked: ``preds`` is ``[B, P_N]`` with tables ``[B, M, T]`` (or
    ``[B, T]``: one tree per source, the results come without ``M``) or ``[P_N]`` with tables ``[M, T]`` (or ``[T]``).  →
    ``(preds float32 [B, P_N], slots int32 [B, M, T], lengths float64 [B, M, T], (B, M, N), (single, one), zeroed (patristic
    or None, rows, worst_j, status))``."""
    p = np.ascontiguousarray(np.asarray(preds, dtype=np.float32))
    s = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
    l = np.ascontiguousarray(np.asarray(lengths, dtype=np.float64))
    single = p.ndim == 1
    if single:
        p, s, l = p[None], s[None], l[None]
    one = s.ndim == 2
    if one:
        s, l = s[:, None, :], l[:, None, :] if l.ndim == 2 else l
    if p.ndim != 2 or s.ndim != 3 or l.shape != s.shape or s.shape[0] != p.shape[0]:
        raise ValueError(f"expected distances [B, P] and tables [B, M, T], got {np.shape(preds)}, {np.shape(slots)} and {np.shape(lengths)}")
    n = n_of_pairs(p.shape[1])
    b, m, t = s.shape
    if n * (n - 1) // 2 != p.shape[1] or (n >= 3 and t != table_len(n)):
        raise ValueError(f"{p.shape[1]} distances and {t} slots are not those of one number of sequences")
    refuse(b, m, n)
    out = (np.zeros((b, m, p.shape[1]), dtype=np.float64) if patristic else None, np.zeros((b, m, n, COLS), dtype=np.float64),
           np.zeros((b, m, n), dtype=np.int32), np.zeros((b, m), dtype=np.uint8))
    return p, s, l, (b, m, n), (single, one), out


def squeezed(out, flags):
    """The results without ``M`` and ``B`` where the arguments came without them."""
    single, one = flags
    if one:
        out = tuple(None if x is None else x[:, 0] for x in out)
    return unbatched(out, single)


# ---- the statement ------------------------------------------------------------------------------------------------------

def table_status(slots: Sequence[int], n: int) -> int:
    """``NO_TABLE`` unless ``slots [T]`` is a join table of ``n`` sequences."""
    s = [int(v) for v in slots]
    alive = [True] * n
    for t in range(n - 3):
        a, b = s[2 * t], s[2 * t + 1]
        if not (0 <= a < n and 0 <= b < n) or a == b or not alive[a] or not alive[b]:
            return NO_TABLE
        alive[b] = False
    last = s[2 * (n - 3):]
    if any(not 0 <= v < n for v in last) or len(set(last)) != 3 or not all(alive[v] for v in last):
        return NO_TABLE
    return OK


def nodes_of(slots: Sequence[int], lengths: Sequence[float], n: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(parent int32 [2n - 2], len float64 [2n - 2])`` of a join table (status 0): what the setup kernel makes.  The last
    node is its own parent, with length 0."""
    parent, blen = np.zeros(2 * n - 2, dtype=np.int32), np.zeros(2 * n - 2, dtype=np.float64)
    node = list(range(n))
    for t in range(n - 3):
        a, b = int(slots[2 * t]), int(slots[2 * t + 1])
        for k, s in enumerate((a, b)):
            parent[node[s]], blen[node[s]] = n + t, lengths[2 * t + k]
        node[a] = n + t
    for k in range(3):
        s = int(slots[2 * (n - 3) + k])
        parent[node[s]], blen[node[s]] = 2 * n - 3, lengths[2 * (n - 3) + k]
    parent[2 * n - 3] = 2 * n - 3
    return parent, blen


def patristic_py(slots: Sequence[int], lengths: Sequence[float], n: int) -> np.ndarray:
    """The tree's distances ``float64 [P_n]`` of a join table (status 0), by the replay with member lists."""
    out = np.zeros(n * (n - 1) // 2, dtype=np.float64)
    members = {s: [s] for s in range(n)}
    h = [0.0] * n

    def lift(group, length):
        for x in group:
            h[x] = h[x] + length

    def unite(left, right):
        for x in left:
            for y in right:
                out[pair_index(min(x, y), max(x, y), n)] = h[x] + h[y]

    for t in range(n - 3):
        a, b = int(slots[2 * t]), int(slots[2 * t + 1])
        left, right = members[a], members.pop(b)
        lift(left, float(lengths[2 * t]))
        lift(right, float(lengths[2 * t + 1]))
        unite(left, right)
        members[a] = left + right
    base = 2 * (n - 3)
    last = [members[int(slots[base + k])] for k in range(3)]
    for k in range(3):
        lift(last[k], float(lengths[base + k]))
    unite(last[0], last[1])
    unite(last[0], last[2])
    unite(last[1], last[2])
    return out


def row_sums_py(pred: np.ndarray, tree: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(rows float64 [n, 6], worst_j int32 [n])`` of the distances ``pred float32 [P_n]`` and the tree's ``tree float64 [P_n]``,
    in the order the module's text defines."""
    d_all, t_all = np.asarray(pred, dtype=np.float32).astype(np.float64).tolist(), np.asarray(tree, dtype=np.float64).tolist()
    rows, worst_j = np.zeros((n, COLS), dtype=np.float64), np.zeros(n, dtype=np.int32)
    for i in range(n):
        acc = [[0.0] * LANES for _ in range(5)]
        worst, where = [-1.0] * LANES, [n] * LANES
        for lane in range(LANES):
            for j in range(lane, n, LANES):
                if j == i:
                    continue
                p = pair_index(min(i, j), max(i, j), n)
                d, t = d_all[p], t_all[p]
                e = d - t
                e2 = e * e
                acc[SS][lane] = acc[SS][lane] + e2
                acc[FM][lane] = acc[FM][lane] + (e2 / (d * d) if d > 0.0 else 0.0)
                acc[ST][lane] = acc[ST][lane] + t
                acc[STT][lane] = acc[STT][lane] + t * t
                acc[SDT][lane] = acc[SDT][lane] + d * t
                if abs(e) > worst[lane]:
                    worst[lane], where[lane] = abs(e), j
        s = LANES // 2
        while s:
            for lane in range(s):
                for a in acc:
                    a[lane] = a[lane] + a[lane + s]
                w, j = worst[lane + s], where[lane + s]
                if w > worst[lane] or (w == worst[lane] and j < where[lane]):
                    worst[lane], where[lane] = w, j
            s //= 2
        rows[i] = [a[0] for a in acc] + [worst[0]]
        worst_j[i] = where[0]
    return rows, worst_j


def tree_fit_py(pred, slots, lengths, n: int):
    """The statement, one source's distances ``pred float32 [P_n]`` and ONE of its trees: ``(patristic float64 [P_n], rows float64
    [n, 6], worst_j int32 [n], status uint8 scalar)``."""
    pred = np.asarray(pred, dtype=np.float32)
    slots, lengths = np.asarray(slots, dtype=np.int32), np.asarray(lengths, dtype=np.float64)
    refuse(1, 1, n)
    pairs = n * (n - 1) // 2
    if pred.shape != (pairs,) or slots.shape != (table_len(n),) or lengths.shape != slots.shape:
        raise ValueError(f"expected {pairs} distances and {table_len(n)} slots and lengths for {n} sequences, got {pred.shape}, "
                         f"{slots.shape} and {lengths.shape}")
    zeros = (np.zeros(pairs, dtype=np.float64), np.zeros((n, COLS), dtype=np.float64), np.zeros(n, dtype=np.int32))
    if table_status(slots, n) != OK:
        return (*zeros, np.uint8(NO_TABLE))
    if not (np.isfinite(pred).all() and np.isfinite(lengths).all()):
        return (*zeros, np.uint8(NONFINITE))
    tree = patristic_py(slots, lengths, n)
    return (tree, *row_sums_py(pred, tree, n), np.uint8(OK))


def tree_fit_batch_py(preds, slots, lengths):
    """``tree_fit_py`` of every tree of every source, with ``Engine.tree_fit``'s arguments and results: the host side of
    ``--python-io`` (``treekinds.PythonHost``)."""
    p, s, l, (b, m, n), flags, out = fit_arrays(preds, slots, lengths)
    for k in range(b):
        for r in range(m):
            for dst, src in zip(out, tree_fit_py(p[k], s[k, r], l[k, r], n)):
                dst[k, r] = src
    return squeezed(out, flags)


# ---- derived in Python only ---------------------------------------------------------------------------------------------

class Scores(NamedTuple):
    """What ``--fit`` reports of one tree; ``nan`` for a tree with a status."""
    ss: float               # the residual sum of squares over the pairs
    rmse: float             # sqrt(ss / P)
    taxon_rms: np.ndarray   # float64 [n]: sqrt(ss[i] / (n - 1))
    explained: float        # 1 - ss / sum (d - mean d)^2; nan for constant distances
    fm: float               # the Fitch-Margoliash sum over the pairs
    correlation: float      # of d and T over the pairs (the cophenetic correlation); nan where either is constant
    worst: Tuple[int, int, float]     # the pair with the largest |e|, i < j, and that |e|


def half_sum(column) -> float:
    """Half of the sum over the sequences, added in their order: every pair is in two rows."""
    total = 0.0
    for x in np.asarray(column, dtype=np.float64).tolist():
        total = total + x
    return total * 0.5


def fit_scores(pred: np.ndarray, rows: np.ndarray, worst_j: np.ndarray, n: int) -> Scores:
    """The derived figures of one tree (status 0) from its ``rows [n, 6]`` and ``worst_j [n]`` and the source's distances."""
    rows = np.asarray(rows, dtype=np.float64).reshape(n, COLS)
    d = np.asarray(pred, dtype=np.float32).astype(np.float64)
    pairs = n * (n - 1) // 2
    ss, fm = half_sum(rows[:, SS]), half_sum(rows[:, FM])
    st, stt, sdt = half_sum(rows[:, ST]), half_sum(rows[:, STT]), half_sum(rows[:, SDT])
    mean_d = float(d.sum()) / pairs
    var_d = float(np.square(d - mean_d).sum())
    mean_t = st / pairs
    var_t = stt - pairs * mean_t * mean_t
    cov = sdt - pairs * mean_d * mean_t
    nan = float("nan")
    i = int(np.argmax(rows[:, WORST]))
    j = int(worst_j[i])
    return Scores(ss, math.sqrt(ss / pairs), np.sqrt(rows[:, SS] / (n - 1)), 1.0 - ss / var_d if var_d > 0 else nan, fm,
                  cov / math.sqrt(var_d * var_t) if var_d > 0 and var_t > 0 else nan, (min(i, j), max(i, j), float(rows[i, WORST])))


def no_scores(n: int) -> Scores:
    """The scores of a tree with a status (distances or lengths that are not finite)."""
    nan = float("nan")
    return Scores(nan, nan, np.full(n, nan), nan, nan, nan, (0, 0, nan))


# ---- the files of --fit -------------------------------------------------------------------------------------------------

FIT_HEAD = "kind\trmse\texplained\tfm\tcorrelation\tworst_i\tworst_j\tworst_residual\n"
TAXA_HEAD = "index\tid\trms_residual\trelative\n"


def fit_line(kind: str, s: Scores) -> str:
    """One kind's line of ``<stem>.fit.tsv``."""
    return f"{kind}\t{s.rmse:.10g}\t{s.explained:.10f}\t{s.fm:.10g}\t{s.correlation:.10f}\t{s.worst[0]}\t{s.worst[1]}\t{s.worst[2]:.10g}\n"


def fit_tsv(lines: Sequence[Tuple[str, Scores]]) -> str:
    """``<stem>.fit.tsv``: one line per written kind."""
    return FIT_HEAD + "".join(fit_line(kind, s) for kind, s in lines)


def taxa_tsv(ids: Sequence[str], s: Scores) -> str:
    """``<stem>.<kind>.fit.taxa.tsv``: per sequence its RMS residual and that over the mean of the sequences' (``nan`` where the
    mean is 0 or there is none)."""
    mean = float(np.mean(s.taxon_rms)) if len(s.taxon_rms) else float("nan")
    lines = [TAXA_HEAD]
    for k, (name, x) in enumerate(zip(ids, s.taxon_rms.tolist())):
        rel = x / mean if mean > 0 else float("nan")
        lines.append(f"{k}\t{name}\t{x:.10g}\t{rel:.10f}\n")
    return "".join(lines)


def parse_fit_tsv(text: str) -> dict:
    """``{kind: (rmse, explained, fm, correlation, worst_i, worst_j, worst_residual)}`` of a ``<stem>.fit.tsv``."""
    out = {}
    for row in text.splitlines()[1:]:
        c = row.split("\t")
        out[c[0]] = (float(c[1]), float(c[2]), float(c[3]), float(c[4]), int(c[5]), int(c[6]), float(c[7]))
    return out
