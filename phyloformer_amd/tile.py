"""Tiled inference on the host: the host twins of ``csrc/pf_tile_host.h`` / ``csrc/pf_tile.hip.h`` and the writer of
``infer_alns.py --tile``.

An alignment of ``N`` sequences beyond what one forward takes is covered by sets of at most ``M`` rows, the CONTEXT a
distance is predicted in (distances are context dependent: ``taxa.py``).  For ``2 <= M < N``:

* ``G = ceil(N / floor(M / 2))`` groups (``G >= 3``); group ``g`` is the contiguous rows
  ``[floor(g N / G), floor((g + 1) N / G))``: sizes differ by at most one;
* set ``(g, h)``, ``g < h``, in lexicographic order, is the rows of group ``g`` followed by the rows of group ``h``:
  ``m = n_g + n_h <= M`` rows and ``m (m - 1) / 2`` distances in the reference's pair order; ``S = G (G - 1) / 2`` sets
  of at most three distinct sizes, ``T`` distances in all;
* a cross-group pair lies in exactly one set, a within-group pair of group ``g`` in the ``G - 1`` sets that contain ``g``.

``combine`` mirrors ``k_tile_combine`` operation for operation - the same double additions in ascending order of the
partner group, one division, one rounding - and is bit-identical to it.  ``spread`` is the standard deviation of a
within-group pair's distance over its ``G - 1`` contexts and exactly 0 for a cross-group pair, which has one context: it
is descriptive, not a test, and 0 there means "not measured".
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import numpy as np


class Plan(NamedTuple):
    N: int
    M: int
    G: int
    bounds: np.ndarray        # int64 [G + 1]: first row of every group, then N
    sets: Tuple[Tuple[int, int], ...]    # (g, h) of every set, in order
    offset: np.ndarray        # int64 [S + 1]: first distance of every set among the T of a source, then T

    @property
    def S(self) -> int:
        return len(self.sets)

    @property
    def T(self) -> int:
        return int(self.offset[-1])

    def rows(self, g: int) -> int:
        return int(self.bounds[g + 1] - self.bounds[g])

    def set_rows(self, k: int) -> np.ndarray:
        """The source rows of set ``k``: group ``g``'s, then group ``h``'s, ascending."""
        g, h = self.sets[k]
        return np.concatenate([np.arange(self.bounds[g], self.bounds[g + 1]), np.arange(self.bounds[h], self.bounds[h + 1])])

    def groups_of_rows(self) -> np.ndarray:
        """``int64[N]``: the group of every row."""
        return np.repeat(np.arange(self.G), np.diff(self.bounds))


def groups(N: int, M: int) -> int:
    """``G`` (``pf_tile_groups``); ``ValueError`` for ``M < 2`` or ``N <= M``."""
    N, M = int(N), int(M)
    if M < 2:
        raise ValueError(f"tiling needs a context of M >= 2 sequences (got {M})")
    if N <= M:
        raise ValueError(f"N={N} sequences fit one context of M={M}: no tiling")
    return -(-N // (M // 2))


def plan(N: int, M: int) -> Plan:
    G = groups(N, M)
    N, M = int(N), int(M)
    bounds = np.array([g * N // G for g in range(G + 1)], dtype=np.int64)
    sets = tuple((g, h) for g in range(G) for h in range(g + 1, G))
    sizes = np.diff(bounds)
    m = np.array([sizes[g] + sizes[h] for g, h in sets], dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(m * (m - 1) // 2)]).astype(np.int64)
    return Plan(N, M, G, bounds, sets, offset)


def _sources(idx) -> np.ndarray:
    idx = np.asarray(idx, dtype=np.uint8)
    if idx.ndim not in (2, 3):
        raise ValueError(f"idx must be [B, N, L] or [N, L], got shape {idx.shape}")
    return idx


def cut_sets(idx: np.ndarray, M: int) -> List[np.ndarray]:
    """``uint8[B, N, L]`` (or ``[N, L]``) → the ``S`` sets in order, set ``k`` as contiguous ``uint8[B, m_k, L]``
    (``[m_k, L]``): ``idx[..., plan.set_rows(k), :]``, what ``k_gather_taxa`` builds on the device."""
    idx = _sources(idx)
    p = plan(idx.shape[-2], M)
    return [np.ascontiguousarray(idx[..., p.set_rows(k), :]) for k in range(p.S)]


def assemble(set_distances: Sequence[np.ndarray]) -> np.ndarray:
    """The sets' distance vectors ``[..., P_m]``, in order, as the ``[..., T]`` layout ``k_tile_combine`` reads."""
    return np.ascontiguousarray(np.concatenate([np.asarray(d, np.float32) for d in set_distances], axis=-1))


def _pidx(i, j, n):
    """Index of pair ``(i, j)``, ``i < j``, among ``n`` rows (int64 arrays)."""
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def _set_index(g: int, h: int, G: int) -> int:
    return g * (2 * G - g - 1) // 2 + (h - g - 1)


def combine(set_distances, N: int, M: int) -> Tuple[np.ndarray, np.ndarray]:
    """``set_distances``: ``float32[..., T]`` or the sequence of the ``S`` sets' ``float32[..., P_m]`` →
    ``(out float32[..., P_N], spread float32[..., P_N])``, the host twin of ``k_tile_combine``, bit for bit."""
    p = plan(N, M)
    flat = set_distances if isinstance(set_distances, np.ndarray) else assemble(set_distances)
    flat = np.asarray(flat, np.float32)
    if flat.shape[-1] != p.T:
        raise ValueError(f"the sets of N={p.N}, M={p.M} hold T={p.T} distances, got {flat.shape[-1]}")
    N, G = p.N, p.G
    lead = flat.shape[:-1]
    out = np.zeros(lead + (N * (N - 1) // 2,), np.float32)
    spread = np.zeros_like(out)                                  # cross-group pairs: exactly 0
    b = p.bounds
    for k, (g, h) in enumerate(p.sets):                          # across groups: a copy
        ng, nh = p.rows(g), p.rows(h)
        il, jl = np.meshgrid(np.arange(ng, dtype=np.int64), np.arange(nh, dtype=np.int64), indexing="ij")
        out[..., _pidx(b[g] + il, b[h] + jl, N)] = flat[..., p.offset[k] + _pidx(il, ng + jl, ng + nh)]
    for g in range(G):                                           # within a group: G - 1 values per pair
        ng = p.rows(g)
        if ng < 2:
            continue
        iu, ju = (a.astype(np.int64) for a in np.triu_indices(ng, k=1))
        vals = []
        for q in range(G):                                       # ascending order of the partner group
            if q == g:
                continue
            nq = p.rows(q)
            src = (p.offset[_set_index(q, g, G)] + _pidx(nq + iu, nq + ju, nq + ng) if q < g else
                   p.offset[_set_index(g, q, G)] + _pidx(iu, ju, ng + nq))
            vals.append(flat[..., src].astype(np.float64))
        total = np.zeros(lead + (len(iu),), np.float64)
        for v in vals:                                           # (not np.sum: its order is not the kernel's)
            total = total + v
        mean = total / np.float64(G - 1)
        ss = np.zeros_like(total)
        for v in vals:
            d = v - mean
            ss = ss + d * d
        dest = _pidx(b[g] + iu, b[g] + ju, N)
        out[..., dest] = mean.astype(np.float32)
        spread[..., dest] = np.sqrt(ss / np.float64(G - 2)).astype(np.float32)
    return out, spread


TSV_COLUMNS = ("index", "id", "group")


def tile_tsv(ids: Sequence[str], M: int) -> str:
    """``<stem>.tile.tsv``: header ``index id group``, one row per sequence (index 0-based) with its group in the plan of
    ``(len(ids), M)``: two sequences share all their contexts when their groups are equal, one context otherwise."""
    grp = plan(len(ids), M).groups_of_rows()
    return "".join(["\t".join(TSV_COLUMNS) + "\n"] + [f"{k}\t{ids[k]}\t{int(grp[k])}\n" for k in range(len(ids))])
