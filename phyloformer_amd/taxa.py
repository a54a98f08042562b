"""The taxon axis on the host: the host twins of ``csrc/pf_taxa.hip.h`` / ``csrc/pf_taxa_host.h`` and the writers of
``infer_alns.py --leave-one-out``.

Phyloformer's distances are context dependent: column attention mixes all pairs, so the predicted distance between A
and B changes when C leaves the alignment.  ``cut_taxa`` mirrors ``k_gather_taxa``: ``Engine.forward_taxa`` promises the
bits of ``Engine.forward(cut_taxa(idx, taxa))``.  ``loo_stats`` mirrors ``k_loo_taxon`` / ``k_loo_pair``.

Pair order (the reference's, the row-major upper triangle): pair ``(i, j)``, ``i < j``, of ``N`` rows has index
``i (2N - i - 1) / 2 + (j - i - 1)``.  Leave-one-out set ``t`` is the alignment without row ``t``, the remaining rows in
order, so pair ``(i, j)`` - neither of them ``t`` - has there the index of ``(i - (i > t), j - (j > t))`` among
``N - 1`` rows.  With ``delta_t(i, j) = loo[t][that index] - full[(i, j)]``:

    influence[t]   = sqrt(mean over the P1 pairs of delta_t^2)          how far removing t moves the others
    shift[t]       = mean over the P1 pairs of delta_t                  signed: did t's presence stretch or shrink them
    context[(i,j)] = sqrt(sum_{t not in {i,j}} delta_t(i,j)^2 / (N-2))  how much the distance depends on the rest

They are descriptive, not a test statistic; two identical sequences have equal ``influence`` by construction.
"""
from __future__ import annotations

from typing import Dict, FrozenSet, Iterable, Optional, Sequence, Tuple

import numpy as np


def pair_index(i: int, j: int, N: int) -> int:
    """Index of pair ``(i, j)``, ``0 <= i < j < N``, in the row-major upper triangle."""
    i, j, N = int(i), int(j), int(N)
    if not 0 <= i < j < N:
        raise ValueError(f"a pair needs 0 <= i < j < N (got i={i}, j={j}, N={N})")
    return i * (2 * N - i - 1) // 2 + (j - i - 1)


def pair_of(q: int, N: int) -> Tuple[int, int]:
    """The pair ``(i, j)`` of index ``q`` among ``N`` rows (the inverse of ``pair_index``)."""
    q, N = int(q), int(N)
    if N < 2 or not 0 <= q < N * (N - 1) // 2:
        raise ValueError(f"pair index {q} is outside [0, {max(N, 0) * (N - 1) // 2}) for N={N}")
    i = 0
    while (i + 1) * (2 * N - i - 2) // 2 <= q:
        i += 1
    return i, i + 1 + q - i * (2 * N - i - 1) // 2


def loo_pair_index(i: int, j: int, t: int, N: int) -> int:
    """Index of pair ``(i, j)`` of the ``N`` rows in the leave-one-out set ``t`` (``N - 1`` rows)."""
    i, j, t, N = int(i), int(j), int(t), int(N)
    if not 0 <= t < N or t in (i, j):
        raise ValueError(f"set t={t} does not hold pair ({i}, {j}) of N={N} rows")
    if not 0 <= i < j < N:
        raise ValueError(f"a pair needs 0 <= i < j < N (got i={i}, j={j}, N={N})")
    return pair_index(i - (i > t), j - (j > t), N - 1)


def leave_one_out_sets(N: int) -> np.ndarray:
    """The taxon table ``int32[N, N - 1]`` of the ``N`` cuts: row ``t`` is ``0 .. N - 1`` without ``t``."""
    N = int(N)
    if N < 3:
        raise ValueError(f"leave-one-out needs N >= 3 sequences (got {N})")
    m = np.arange(N - 1, dtype=np.int32)[None, :]
    return (m + (m >= np.arange(N, dtype=np.int32)[:, None])).astype(np.int32)


def cut_taxa(idx: np.ndarray, taxa: np.ndarray) -> np.ndarray:
    """``uint8[B, N, L]``, ``int[S, M]`` → ``uint8[B, S, M, L]`` (``[N, L]`` → ``[S, M, L]``): derived alignment ``s`` of
    source ``b`` is ``idx[b][taxa[s], :]``.  Entries outside ``[0, N)`` raise ``ValueError`` (never wrapped)."""
    idx = np.asarray(idx, dtype=np.uint8)
    tab = np.asarray(taxa)
    if idx.ndim not in (2, 3):
        raise ValueError(f"idx must be [B, N, L] or [N, L], got shape {idx.shape}")
    if tab.ndim != 2 or tab.dtype.kind not in "iu":
        raise ValueError(f"taxa must be an integer array [S, M], got {tab.dtype} {tab.shape}")
    N = idx.shape[-2]
    if tab.size and (tab.min() < 0 or tab.max() >= N):
        raise ValueError(f"taxon outside [0, {N})")
    return np.ascontiguousarray(idx[..., tab, :])


def _loo_map(N: int) -> np.ndarray:
    """``int64[N, P1]``: the full-alignment pair index of every pair of every leave-one-out set."""
    P1 = (N - 1) * (N - 2) // 2
    out = np.empty((N, P1), np.int64)
    iu, ju = np.triu_indices(N - 1, k=1)                       # row-major upper triangle of N - 1 rows
    for t in range(N):
        i, j = iu + (iu >= t), ju + (ju >= t)
        out[t] = i * (2 * N - i - 1) // 2 + (j - i - 1)
    return out


def loo_stats(full: np.ndarray, loo: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``full [..., P]``, ``loo [..., N, P1]`` → ``(influence [..., N], shift [..., N], context [..., P])``: the literal
    definitions in float64, rounded to float32 once."""
    f = np.asarray(full, np.float64)
    lo = np.asarray(loo, np.float64)
    if lo.ndim < 2 or f.ndim != lo.ndim - 1 or f.shape[:-1] != lo.shape[:-2]:
        raise ValueError(f"full is [..., P] and loo [..., N, P1], got {f.shape} and {lo.shape}")
    N, P1 = lo.shape[-2:]
    if N < 3 or P1 != (N - 1) * (N - 2) // 2 or f.shape[-1] != N * (N - 1) // 2:
        raise ValueError(f"shapes {f.shape} and {lo.shape} are not those of N >= 3 sequences")
    fmap = _loo_map(N)
    delta = lo - f[..., fmap]                                  # [..., N, P1]
    influence = np.sqrt((delta ** 2).mean(axis=-1))
    shift = delta.mean(axis=-1)
    ssq = np.zeros(f.shape, np.float64)
    for t in range(N):                                         # t in index order, as k_loo_pair
        ssq[..., fmap[t]] += delta[..., t, :] ** 2
    context = np.sqrt(ssq / (N - 2))
    return influence.astype(np.float32), shift.astype(np.float32), context.astype(np.float32)


def restrict_splits(sp: Dict[FrozenSet[str], float], leaf: str, leaves: Iterable[str]) -> Dict[FrozenSet[str], float]:
    """``treecmp.splits`` of a tree over ``leaves`` with ``leaf`` pruned: the leaf is dropped from every split, splits
    that became trivial (one leaf, or all but one, of the remaining) are discarded, two splits that became the same one
    add their lengths.  Keys follow ``treecmp.splits``' rule on the remaining leaves: the side without their smallest
    name (``leaves`` is needed for that: no key of ``sp`` names the smallest leaf)."""
    universe = set(leaves)
    if leaf not in universe:
        raise ValueError(f"leaf {leaf!r} is not in the tree")
    rest = frozenset(universe) - {leaf}
    if not rest:
        return {}
    anchor = min(rest)
    out: Dict[FrozenSet[str], float] = {}
    for side, length in sp.items():
        side = frozenset(side) - {leaf}
        if anchor in side:
            side = rest - side
        if 1 < len(side) < len(rest) - 1:
            out[side] = out.get(side, 0.0) + length
    return out


TSV_COLUMNS = ("index", "id", "influence", "shift", "relative")


def taxa_tsv(ids: Sequence[str], influence: np.ndarray, shift: np.ndarray, rf_pruned: Optional[Sequence[object]] = None) -> str:
    """``<stem>.taxa.tsv``: header ``index id influence shift relative`` (``rf_pruned`` too when given), one row per
    sequence (index 0-based); ``relative = influence / mean(influence)``, ``NA`` when the mean is 0.  ``influence`` and
    ``shift`` have the number format of ``<stem>.phy``, ``relative`` that of ``<stem>.sites.tsv``."""
    inf = np.asarray(influence, np.float64).reshape(-1)
    sh = np.asarray(shift, np.float64).reshape(-1)
    mean = float(inf.mean()) if inf.size else 0.0
    cols = TSV_COLUMNS + (("rf_pruned",) if rf_pruned is not None else ())
    rows = ["\t".join(cols) + "\n"]
    for k in range(inf.size):
        rel = "NA" if mean == 0.0 else f"{float(inf[k]) / mean:.15f}"
        row = f"{k}\t{ids[k]}\t{float(inf[k]):.10f}\t{float(sh[k]):.10f}\t{rel}"
        if rf_pruned is not None:
            row += f"\t{rf_pruned[k]}"
        rows.append(row + "\n")
    return "".join(rows)


def rf_pruned(full_tree: str, loo_trees: Sequence[str], N: int) -> list:
    """Per ``t``: the Robinson-Foulds distance between the tree of set ``t`` (``loo_trees[t]``) and the whole alignment's
    tree restricted to the remaining taxa.  The trees carry index labels ``"0" .. "N-1"`` (set ``t``: without ``t``), so
    duplicate sequence ids do not matter.  ``"NA"`` when ``N - 1 < 4``: such trees have no internal split."""
    from .treecmp import _internal, parse_newick, splits
    if N - 1 < 4:
        return ["NA"] * N
    labels = [str(k) for k in range(N)]
    full = splits(parse_newick(full_tree))
    out = []
    for t in range(N):
        want = set(restrict_splits(full, labels[t], labels))
        got = _internal(splits(parse_newick(loo_trees[t])), N - 1)
        out.append(len(want ^ got))
    return out


def context_phylip(context: np.ndarray, ids: Sequence[str]) -> str:
    """``<stem>.context.phy``: the context values as a PHYLIP matrix, ids and number format of ``<stem>.phy``."""
    from .phylip import vec_to_phylip
    return vec_to_phylip(np.asarray(context), ids)[1]
