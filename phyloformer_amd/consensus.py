"""Majority-rule consensus of the replicate trees of a bootstrap, with split frequencies and mean branch lengths, for the
``--consensus`` argument of the CLI's ``--bootstrap`` mode.  DESIGN.md section 25.

This module is the readable statement and the yardstick of the native code (``csrc/pf_consensus_host.h``,
``csrc/pf_consensus.hip.h``): brute force, Python ints as bitsets, in the style of ``supports.py``.

**Inputs.**  ``R >= 1`` replicate join tables ``rep_slots int32 [R][T]``, ``T = 2 (N - 3) + 3``, ``N >= 4``; optionally
their lengths ``rep_lengths float64 [R][T]`` and flags ``rep_flag [R]``; a threshold ``F``, an integer percent in
``50 .. 99``.  A flagged replicate has no tree: its table is never read and it contains no split, but it counts in ``R``.
``V`` is the number of unflagged replicates.

**Splits and counts.**  The splits of a table are ``supports.table_splits`` (``N - 3`` per tree, the side without sequence
0, distinct within a tree); ``c(s)`` = the unflagged replicates whose tree contains ``s``.

**Selection.**  ``s`` is selected iff ``100 c(s) > F R``, strictly.  With ``F >= 50`` the selected splits are pairwise
compatible - none contains sequence 0, so any two are disjoint or nested - and there are ``M <= N - 3`` of them.

**Canonical order.**  By ``(size, lowest member)`` ascending: two compatible clusters with one lowest member are nested,
two nested clusters of one size are equal - a total order that does not depend on how the splits were found.

**Tree.**  ``parent[i]`` = the least ``j > i`` with ``split_j >= split_i`` (as sets), or -1 (the root);
``leaf_parent[x]`` = the least ``j`` with ``x in split_j``, or -1.  Leaf 0 always hangs from the root.

**Lengths** (where given).  ``lengths[p]`` of a table is the branch above the cluster that sits in ``slots[p]`` at that
point: the branch above join ``t``'s cluster is at the first ``p > 2 t + 1`` with ``slots[p] == slots[2 t]``, the branch
above leaf ``x`` at the first ``p`` with ``slots[p] == x``.  ``split_length[i]`` = the sum over the replicates that
contain split ``i``, in ascending replicate order, in float64, divided by ``c``; ``leaf_length[x]`` = the same sum over all
unflagged replicates divided by ``V`` (0.0 where ``V = 0``).  The order is fixed and there is no product, so the device,
its serial twin and this statement agree bit for bit.

**Status.**  0; 1 where an unflagged table is no join table - every result is then zero.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

from .bootstrap import support_percent
from .supports import table_splits
from .treekinds import NJ_STARTED

# From this many sequences on the CLI builds a sub-batch's consensus trees on the GPU thread (``Engine.join_consensus``)
# instead of on the writer threads' serial twin.  A measured constant by ``supports.SUPPORT_DEVICE_MIN``'s rule (DESIGN.md
# section 25, tools/consensus_bench.py, profiles/consensus_bench.txt): the smallest measured N at which the device side
# takes at most half the host's time at R = 100; None = the device path is off in the CLI (the API stays).
CONSENSUS_DEVICE_MIN = 1024

PERCENT_MIN, PERCENT_MAX = 50, 99
# the file of a kind's consensus tree (supports.SUFFIXES' kinds)
SUFFIXES = {k.name: k.files("con.nwk")[0] for k in NJ_STARTED}


class Consensus(NamedTuple):
    """One source's consensus: the first ``n_splits`` entries of the ``[N - 3]`` lists are valid, zeros beyond;
    ``split_length`` / ``leaf_length`` are None without lengths."""
    n_splits: int
    count: List[int]
    size: List[int]
    parent: List[int]
    split_length: Optional[List[float]]
    leaf_parent: List[int]
    leaf_length: Optional[List[float]]
    status: int


def check_percent(percent) -> int:
    if int(percent) != percent or not PERCENT_MIN <= int(percent) <= PERCENT_MAX:
        raise ValueError(f"the consensus threshold is an integer percent from {PERCENT_MIN} to {PERCENT_MAX} (got {percent})")
    return int(percent)


def branch_positions(slots: Sequence[int], n: int):
    """``(above [n - 3], leaf_pos [n])``: where a valid table's lengths hold the branch above every join's cluster and
    above every leaf (module docstring), found by the definition's own scans."""
    slots = [int(s) for s in slots]
    above = [next(p for p in range(2 * t + 2, len(slots)) if slots[p] == slots[2 * t]) for t in range(n - 3)]
    leaf_pos = [slots.index(x) for x in range(n)]
    return above, leaf_pos


def _zeros(n: int, lengths: bool, status: int) -> Consensus:
    s = n - 3
    return Consensus(0, [0] * s, [0] * s, [0] * s, [0.0] * s if lengths else None, [0] * n, [0.0] * n if lengths else None, status)


def join_consensus(rep_slots: Sequence[Sequence[int]], n: int, rep_lengths: Optional[Sequence[Sequence[float]]] = None,
                   rep_flag: Optional[Sequence[bool]] = None, percent: int = 50) -> Consensus:
    """One source's majority-rule consensus (module docstring)."""
    R = len(rep_slots)
    if R < 1:
        raise ValueError("a consensus needs R >= 1 replicates")
    if n < 4:
        raise ValueError(f"a consensus needs N >= 4 sequences (got {n})")
    F = check_percent(percent)
    flags = [False] * R if rep_flag is None else [bool(f) for f in rep_flag]
    if len(flags) != R or (rep_lengths is not None and len(rep_lengths) != R):
        raise ValueError(f"expected {R} replicate flags and length rows")
    try:
        trees = [None if f else table_splits(s, n) for s, f in zip(rep_slots, flags)]
    except ValueError:
        return _zeros(n, rep_lengths is not None, 1)
    count = {}
    for splits in trees:
        assert splits is None or len(set(splits)) == n - 3
        for s in splits or ():
            count[s] = count.get(s, 0) + 1
    chosen = [s for s, c in count.items() if 100 * c > F * R]
    assert len(chosen) <= n - 3
    assert all(a & b == 0 or a & b == a or a & b == b for a in chosen for b in chosen)
    size = lambda s: bin(s).count("1")
    low = lambda s: (s & -s).bit_length() - 1
    chosen.sort(key=lambda s: (size(s), low(s)))
    M, S = len(chosen), n - 3
    pad = [0] * (S - M)
    parent = [next((j for j in range(i + 1, M) if chosen[j] & chosen[i] == chosen[i]), -1) for i in range(M)]
    leaf_parent = [next((j for j in range(M) if chosen[j] >> x & 1), -1) for x in range(n)]
    split_length = leaf_length = None
    if rep_lengths is not None:
        where = [None if splits is None else branch_positions(rep_slots[r], n) for r, splits in enumerate(trees)]
        split_length = []
        for s in chosen:
            total = 0.0
            for r, splits in enumerate(trees):
                if splits is not None and s in splits:
                    total += float(rep_lengths[r][where[r][0][splits.index(s)]])
            split_length.append(total / count[s])
        V = sum(splits is not None for splits in trees)
        leaf_length = []
        for x in range(n):
            total = 0.0
            for r, splits in enumerate(trees):
                if splits is not None:
                    total += float(rep_lengths[r][where[r][1][x]])
            leaf_length.append(total / V if V else 0.0)
        split_length += [0.0] * (S - M)
    return Consensus(M, [count[s] for s in chosen] + pad, [size(s) for s in chosen] + pad, parent + pad, split_length,
                     leaf_parent, leaf_length, 0)


def star(n: int, lengths: bool = False) -> Consensus:
    """The unresolved tree of ``n`` leaves (fewer than four sequences, or no replicate with a tree)."""
    s = max(n - 3, 0)
    return Consensus(0, [0] * s, [0] * s, [0] * s, [0.0] * s if lengths else None, [-1] * n, [0.0] * n if lengths else None, 0)


def newick_of_consensus(ids: Sequence[str], results, R: int, clamp_negative: bool = True) -> str:
    """The consensus as text: the root's children are leaf 0 and everything with parent -1, each node's children ordered
    by lowest member; an internal node is ``(children)LABEL:length`` with ``LABEL = bootstrap.support_percent(count, R)``;
    numbers as ``nj.newick_of_joins`` writes them, a negative mean clamped here; no ``:length`` parts without lengths."""
    n_splits, count, _size, parent, split_length, leaf_parent, leaf_length = tuple(results)[:7]
    M, n = int(n_splits), len(ids)

    def fmt(x) -> str:
        x = float(x)
        if clamp_negative and x < 0:
            x = 0.0
        return ":" + repr(x)

    with_lengths = split_length is not None and leaf_length is not None
    # (lowest member, text) of the children of every node; node M is the root
    kids: List[list] = [[] for _ in range(M + 1)]
    for x in range(n):
        kids[int(leaf_parent[x]) if x else -1].append((x, str(ids[x]) + (fmt(leaf_length[x]) if with_lengths else "")))
    # (a parent has a larger rank than its children: ascending ranks close every node before its parent needs it)
    for i in range(M):
        inner = sorted(kids[i])
        text = "(" + ",".join(t for _x, t in inner) + ")" + str(support_percent(int(count[i]), R))
        kids[int(parent[i])].append((inner[0][0], text + (fmt(split_length[i]) if with_lengths else "")))
    return "(" + ",".join(t for _x, t in sorted(kids[M])) + ");\n"
