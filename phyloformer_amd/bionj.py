"""BIONJ (Gascuel 1997) for the ``--bionj`` flag of the CLI: neighbour joining with a matrix of variances beside the
distances and one weight ``lambda`` per join, FastME's default start tree (``fastme -i x.phy``, ``-m I``).  DESIGN.md
section 26.

This module is the readable statement of the algorithm and the yardstick of the native code
(``csrc/pf_bionj_host.h``, ``csrc/pf_bionj.hip.h``): the same float64 operations in the same order, so the tables are
bit-identical.  Pinned against FastME ``-m I`` (tests/golden/fastme_bionj.json, tests/test_bionj.py).  The table is
``nj.nj_joins``' (``nj.Join`` / ``nj.Final``), so ``nj.newick_of_joins``, ``bme.bme_nni`` / ``bme.bme_spr``,
``nj.join_splits``, the supports and the consensus take it unchanged.

Join ``t`` has ``m = N - t`` active positions ``0 .. m-1``; ``active[p]`` is the ROW of ``d`` and ``v`` that position
``p`` lives in (ascending) and ``label[row]`` the smallest sequence of the cluster in that row, its slot in the table:

* **Row sums** ``r``: ``nj.nj_joins``' (numpy's pairwise sum over the active sub-matrix, diagonal included).
* **Criterion**, one orientation only: ``q(x, y) = ((m - 2) d_xy - r[x]) - r[y]`` for positions ``y < x``.
* **Pick** (the windowed rule): the pairs are scanned ``(1,0), (2,0), (2,1), (3,0), ...`` - ``x`` ascending outside,
  ``y`` ascending inside; ``q*`` is the exact minimum over all of them, and the join is the FIRST pair of the scan with
  ``q <= q* + EPS``.  Two minima of total orders (``q``; then the scan index ``x (x - 1) / 2 + y`` over the window), so
  the result does not depend on how the pairs are split among threads.  Near-ties of ``q`` at rounding level
  (duplicated sequences, and the two complementary pairs of the last four clusters) are broken as FastME breaks them.
* **Where the cluster lives.**  The joined cluster takes the row of the LATER position ``x`` and position ``y`` leaves
  the list, as in Gascuel's program: a cluster's row is its largest sequence, and that is what orders the scan of
  later joins.  The table names clusters as ``nj.nj_joins`` does, by their smallest sequence:
  ``label[row x] = min(label[row y], label[row x])``, and the join is written with the smaller label first
  (``a < b``, the new cluster takes slot ``a``), each length beside its own cluster.
* **Lengths**: ``ly = 0.5 d_xy + (r[y] - r[x]) / (2 (m - 2))``, ``lx = d_xy - ly``: ``nj.nj_joins``' formulas on positions.
* **Variances** ``v`` start as a copy of ``d``.
* **Weight** (of ``y``'s row): ``lambda = 0.5`` if ``v_xy == 0``, else ``0.5 + s / ((2 (m - 2)) v_xy)`` with ``s`` the sum
  of ``v_xk - v_yk`` over the active positions ``k`` in active order - positions ``y`` and ``x`` contribute ``0.0`` - in
  numpy's pairwise order, which depends on ``m`` alone; then clamped: not ``>= 0`` gives 0, ``> 1`` gives 1.
* **Updates** for every row ``k`` (``om = 1 - lambda``, ``c = (lambda om) v_xy``):
  ``d_uk = lambda (d_yk - ly) + om (d_xk - lx)``; ``v_uk = (lambda v_yk + om v_xk) - c``; both written to row and
  column ``active[x]``, zero on the diagonal.
* **Final three**: ``nj.nj_joins``' formulas on the three remaining rows in active order, written in ascending order of
  their labels.

Finite input only (the callers send non-finite distances to the NJ text, as ``--bme`` does).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .nj import Final, Join, neighbor_joining, newick_of_joins, table_of_joins

# the window of the pick: the first pair of the scan whose q is within EPS of the exact minimum (absolute, in units of
# Q: substitutions per site times m - 2).  Every value in [1e-12, 5e-9] reproduces FastME on the test data.
EPS = 1e-9

# From this many sequences on the CLI joins a launch's BIONJ trees on the GPU thread (``Engine.bionj_joins``) instead of
# on the writer threads' host code.  A measured constant by section 20's rule (DESIGN.md section 26,
# tools/bionj_bench.py, profiles/bionj_bench.txt): the smallest measured N at which the device takes at most half the
# host's time, never below 201; None = the device path is off in the CLI (the API stays).
BIONJ_DEVICE_MIN: Optional[int] = 512


def pick(q: np.ndarray) -> Tuple[int, int]:
    """The windowed rule on the criterion matrix ``q [m][m]`` (its strict lower triangle is read): positions
    ``(y, x)``, ``y < x``."""
    xs, ys = np.tril_indices(q.shape[0], -1)                # (1,0), (2,0), (2,1), (3,0), ...: the scan order
    qs = q[xs, ys]
    first = int(np.argmax(qs <= qs.min() + EPS))
    return int(ys[first]), int(xs[first])


def weight(vrow_y: np.ndarray, vrow_x: np.ndarray, vxy: float, py: int, px: int) -> float:
    """``lambda`` of a join from the rows of positions ``y`` and ``x`` of the active sub-matrix of variances."""
    if vxy == 0.0:
        return 0.5
    m = vrow_y.shape[0]
    terms = vrow_x - vrow_y
    terms[py] = 0.0
    terms[px] = 0.0
    lam = 0.5 + float(np.sum(terms)) / ((2 * (m - 2)) * vxy)
    if not lam >= 0.0:
        return 0.0
    return 1.0 if lam > 1.0 else lam


def bionj_joins(dm: np.ndarray, trace: Optional[list] = None) -> Tuple[List[Join], Final]:
    """The join sequence of BIONJ on the symmetric ``dm`` (``n >= 3``), float64.  ``trace``, when a list, receives
    ``(lambda, v_xy, number of pairs inside the window)`` of every join."""
    d = np.array(dm, dtype=np.float64)
    v = d.copy()
    n = d.shape[0]
    joins: List[Join] = []
    active = list(range(n))
    label = list(range(n))
    while len(active) > 3:
        m = len(active)
        sub = d[np.ix_(active, active)]
        r = sub.sum(axis=1)
        with np.errstate(all="ignore"):
            q = ((m - 2) * sub - r[:, None]) - r[None, :]       # read at [x][y], y < x
            py, px = pick(q)
            ry, rx = active[py], active[px]
            dxy = sub[px, py]
            ly = 0.5 * dxy + (r[py] - r[px]) / (2 * (m - 2))
            lx = dxy - ly
            vxy = v[rx, ry]
            lam = weight(v[ry, active], v[rx, active], vxy, py, px)
            om = 1.0 - lam
            dn = lam * (d[ry, :] - ly) + om * (d[rx, :] - lx)
            vn = (lam * v[ry, :] + om * v[rx, :]) - (lam * om) * vxy
        if label[ry] < label[rx]:
            joins.append((label[ry], label[rx], float(ly), float(lx)))
        else:
            joins.append((label[rx], label[ry], float(lx), float(ly)))
        if trace is not None:
            xs, ys = np.tril_indices(m, -1)
            qs = q[xs, ys]
            trace.append((lam, float(vxy), int(np.count_nonzero(qs <= qs.min() + EPS))))
        d[rx, :] = dn
        d[:, rx] = dn
        d[rx, rx] = 0.0
        v[rx, :] = vn
        v[:, rx] = vn
        v[rx, rx] = 0.0
        label[rx] = min(label[ry], label[rx])
        active.pop(py)
    i, j, k = active
    li = 0.5 * (d[i, j] + d[i, k] - d[j, k])
    lj = 0.5 * (d[i, j] + d[j, k] - d[i, k])
    lk = 0.5 * (d[i, k] + d[j, k] - d[i, j])
    (i, li), (j, lj), (k, lk) = sorted([(label[i], float(li)), (label[j], float(lj)), (label[k], float(lk))])
    return joins, (i, j, k, li, lj, lk)


def bionj_table(dm: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``bionj_joins`` as ``(slots int32, lengths float64) [2 (N - 3) + 3]``, the layout of ``pf_bionj_joins``."""
    return table_of_joins(*bionj_joins(dm))


def bionj_start(dm: np.ndarray) -> np.ndarray:
    """The slots of ``bionj_joins``' table of ``dm``: a start table for ``bme.bme_nni`` / ``bme.bme_spr``."""
    return bionj_table(dm)[0]


def bionj_newick_py(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> str:
    """``<stem>.bionj.nwk``: the BIONJ tree of ``preds float32 [P_n]``.  Fewer than three sequences have no table and
    non-finite distances no defined tree: the NJ text."""
    from .bme import matrix_of_preds
    n = len(ids)
    dm = matrix_of_preds(preds, n)
    if n < 3 or not np.isfinite(dm).all():
        return neighbor_joining(dm, ids, clamp_negative)
    joins, final = bionj_joins(dm)
    return newick_of_joins(ids, joins, final, clamp_negative)


def _refined_py(search, preds: np.ndarray, ids: Sequence[str], clamp_negative: bool) -> str:
    from .bme import matrix_of_preds, table_to_joins
    n = len(ids)
    dm = matrix_of_preds(preds, n)
    if n < 3 or not np.isfinite(dm).all():
        return neighbor_joining(dm, ids, clamp_negative)
    slots, lengths, _steps, _length, _status = search(dm, bionj_start(dm))
    return newick_of_joins(ids, *table_to_joins(slots, lengths), clamp_negative)


def bionj_bme_newick_py(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> str:
    """``<stem>.bionj.bme.nwk``: ``bme.bme_nni`` started from the BIONJ tree (FastME's ``-n B`` without ``-m``)."""
    from .bme import bme_nni
    return _refined_py(bme_nni, preds, ids, clamp_negative)


def bionj_spr_newick_py(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> str:
    """``<stem>.bionj.spr.nwk``: ``bme.bme_spr`` started from the BIONJ tree (FastME's ``-s`` without ``-m``)."""
    from .bme import bme_spr
    return _refined_py(bme_spr, preds, ids, clamp_negative)
