"""Neighbour joining (Saitou & Nei 1987) for the ``--trees`` flag of the CLI.

The reference delegates to ``skbio.tree.nj`` (/root/reference/infer_alns.py:62-64,
120-123); scikit-bio is not installed in this image, so the tree TEXT of skbio
is unpinned, but the algorithm is pinned against a reference-held neighbour
joining: FastME ``-m N`` from the reference checkout gives the same topology
(RF = 0) and, without clamping, the same branch lengths (<= 3e-8) on the reference's own distance
matrices of all 20 test MSAs (tests/golden/nj_fastme.json,
tests/test_treecmp.py::test_nj_matches_fastme_nj_goldens).  This is the textbook
algorithm with the scikit-bio defaults the reference relies on: negative branch
lengths are clamped to zero and the final three clusters are joined at a
trifurcating root.
O(N³) on N ≤ 200 taxa — host work, not on the device path.

``nj_joins`` is the algorithm (the join sequence), ``newick_of_joins`` the text; ``neighbor_joining`` is the two in a
row, and ``bootstrap.support_newick_py`` reuses both (with ``join_splits``) to label a tree with split supports.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

# one join of two active clusters (slot a < slot b; the new cluster takes slot a) and their branch lengths
Join = Tuple[int, int, float, float]
# the final trifurcation: the three remaining slots and their branch lengths
Final = Tuple[int, int, int, float, float, float]


def nj_joins(dm: np.ndarray) -> Tuple[List[Join], Final]:
    """The join sequence of neighbour joining on ``dm`` (``n >= 3``), float64, ties to the first minimum of ``Q`` in
    row-major order (``np.argmin``)."""
    d = np.array(dm, dtype=np.float64)
    n = d.shape[0]
    joins: List[Join] = []
    active = list(range(n))
    while len(active) > 3:
        m = len(active)
        sub = d[np.ix_(active, active)]
        r = sub.sum(axis=1)
        q = (m - 2) * sub - r[:, None] - r[None, :]
        np.fill_diagonal(q, np.inf)
        a, b = np.unravel_index(np.argmin(q), q.shape)
        if a > b:
            a, b = b, a
        ia, ib = active[a], active[b]
        dab = sub[a, b]
        la = 0.5 * dab + (r[a] - r[b]) / (2 * (m - 2))
        lb = dab - la
        joins.append((ia, ib, la, lb))
        # distances from the new node to every other active node
        dn = 0.5 * (d[ia, :] + d[ib, :] - dab)
        d[ia, :] = dn
        d[:, ia] = dn
        d[ia, ia] = 0.0
        active.pop(b)
    i, j, k = active
    li = 0.5 * (d[i, j] + d[i, k] - d[j, k])
    lj = 0.5 * (d[i, j] + d[j, k] - d[i, k])
    lk = 0.5 * (d[i, k] + d[j, k] - d[i, j])
    return joins, (i, j, k, li, lj, lk)


def table_of_joins(joins: Sequence[Join], final: Final) -> Tuple[np.ndarray, np.ndarray]:
    """A join sequence as ``(slots int32, lengths float64) [2 (N - 3) + 3]``, the layout of ``pf_nj_joins``."""
    slots = np.array([s for a, b, _la, _lb in joins for s in (a, b)] + list(final[:3]), dtype=np.int32)
    lengths = np.array([x for _a, _b, la, lb in joins for x in (la, lb)] + list(final[3:]), dtype=np.float64)
    return slots, lengths


def join_splits(joins: Sequence[Join], n: int) -> List[int]:
    """The split every join creates, as a bitmask over sequence indices, normalised to the side without sequence 0."""
    members = [1 << i for i in range(n)]
    full = (1 << n) - 1
    out = []
    for a, b, _la, _lb in joins:
        members[a] |= members[b]
        s = members[a]
        out.append(s ^ full if s & 1 else s)
    return out


def newick_of_joins(ids: Sequence[str], joins: Sequence[Join], final: Final, clamp_negative: bool = True,
                    support: Optional[Sequence[int]] = None) -> str:
    """Newick text of a join sequence; ``support[t]``, when given, is written after the ``)`` of join ``t``'s node."""
    labels: List[str] = [str(i) for i in ids]

    def fmt(x: float) -> str:
        if clamp_negative and x < 0:
            x = 0.0
        return repr(float(x))

    for t, (ia, ib, la, lb) in enumerate(joins):
        tag = "" if support is None else str(int(support[t]))
        labels[ia] = f"({labels[ia]}:{fmt(la)},{labels[ib]}:{fmt(lb)}){tag}"
    i, j, k, li, lj, lk = final
    return f"({labels[i]}:{fmt(li)},{labels[j]}:{fmt(lj)},{labels[k]}:{fmt(lk)});\n"


def neighbor_joining(dm: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> str:
    """Return a Newick string (terminated by ``;`` and a newline)."""
    d = np.array(dm, dtype=np.float64)
    n = d.shape[0]
    if d.shape != (n, n) or len(ids) != n:
        raise ValueError("distance matrix must be square and match ids")
    if n == 1:
        return f"({ids[0]});\n"
    if n == 2:
        return f"({ids[0]}:{d[0, 1] / 2:.6g},{ids[1]}:{d[0, 1] / 2:.6g});\n"
    joins, final = nj_joins(d)
    return newick_of_joins(ids, joins, final, clamp_negative)
