"""Split supports of join tables: Felsenstein's count and the transfer bootstrap expectation (TBE; Lemoine et al. 2018)
for the ``--tbe`` and ``--bootstrap-refined`` flags of the CLI.  DESIGN.md section 23.

This module is the readable statement and the yardstick of the native code (``csrc/pf_support_host.h``,
``csrc/pf_support.hip.h``): brute force, Python ints as bitsets.  Nothing here is floating point.

**Splits.**  Every tree this project writes (NJ, BNNI, SPR) is a join table ``slots int32 [2 (N - 3) + 3]``; join ``t``
gives the split of its cluster, normalised to the side without sequence 0 (``nj.join_splits``).  A tree has ``N - 3``
splits; split ``t`` has ``k_t`` sequences and depth ``p_t = min(k_t, N - k_t)`` (``>= 2``).

**Transfer distance** of reference split ``s`` (depth ``p``) to a replicate tree with splits ``q_0 .. q_{N-4}``:
``h_j = popcount(s xor q_j)`` and ``delta = min(p - 1, min_j min(h_j, N - h_j))`` - how many sequences have to move for
the split to appear; ``p - 1`` is what the replicate's leaf edges give.  A replicate whose flag is set (it has no tree:
non-finite distances) contributes ``delta = p - 1`` and contains no split.

**Per reference split:** ``count[t]`` = replicates with ``delta = 0`` (what ``<stem>.sup.nwk`` counts),
``transfer[t]`` = the sum of ``delta`` over the replicates, ``depth[t] = p_t``.

**Labels.**  Felsenstein: ``bootstrap.support_percent(count, R)``.  TBE: with ``D = R (p - 1)``,
``tbe_percent = (200 (D - S) + D) // (2 D)`` - ``1 - S / D`` in percent, rounded half up, in integers.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .bme import Tree, table_to_joins
from .bootstrap import support_percent
from .nj import join_splits, newick_of_joins

# From this many sequences on the CLI matches a sub-batch's supports on the GPU thread (``Engine.join_supports``)
# instead of on the writer threads' serial twin.  A measured constant by ``bme.BME_DEVICE_MIN``'s rule (DESIGN.md
# section 23, tools/support_bench.py, profiles/support_bench.txt): the smallest measured N at which the device side
# takes at most half the host's time at R = 100; None = the device path is off in the CLI (the API stays).
SUPPORT_DEVICE_MIN = 200


def table_splits(slots: Sequence[int], n: int) -> List[int]:
    """The ``n - 3`` splits of a join table (``ValueError`` if it is none), as ``nj.join_splits`` gives them."""
    slots = [int(s) for s in slots]
    if n < 4:
        raise ValueError(f"split supports need N >= 4 sequences (got {n})")
    Tree(slots, n)                                              # validates
    return join_splits([(slots[2 * t], slots[2 * t + 1], 0.0, 0.0) for t in range(n - 3)], n)


def split_supports(ref_slots: Sequence[int], rep_slots: Sequence[Sequence[int]], n: int,
                   rep_flag: Optional[Sequence[bool]] = None) -> Tuple[List[int], List[int], List[int]]:
    """One source: ``(count, transfer, depth)``, each ``[n - 3]``, of the reference table over the ``R >= 1`` replicate
    tables (module docstring).  The table of a flagged replicate is not read."""
    if len(rep_slots) < 1:
        raise ValueError("split supports need R >= 1 replicates")
    flags = [False] * len(rep_slots) if rep_flag is None else [bool(f) for f in rep_flag]
    if len(flags) != len(rep_slots):
        raise ValueError(f"expected {len(rep_slots)} replicate flags, got {len(flags)}")
    ref = table_splits(ref_slots, n)
    reps = [None if f else table_splits(s, n) for s, f in zip(rep_slots, flags)]
    count, transfer, depth = [], [], []
    for s in ref:
        k = bin(s).count("1")
        p = min(k, n - k)
        c = total = 0
        for splits in reps:
            delta = p - 1
            for q in splits or ():
                h = bin(s ^ q).count("1")
                delta = min(delta, h, n - h)
            c += delta == 0
            total += delta
        count.append(c)
        transfer.append(total)
        depth.append(p)
    return count, transfer, depth


def tbe_percent(S: int, R: int, p: int) -> int:
    """``1 - S / (R (p - 1))`` in percent, rounded half up."""
    D = int(R) * (int(p) - 1)
    return (200 * (D - int(S)) + D) // (2 * D)


def labels_of(count: Sequence[int], transfer: Sequence[int], depth: Sequence[int], R: int) -> Tuple[List[int], List[int]]:
    """``(Felsenstein percent, TBE percent)`` of every split."""
    return ([support_percent(c, R) for c in count], [tbe_percent(s, R, p) for s, p in zip(transfer, depth)])


def support_texts(slots: Sequence[int], lengths: Sequence[float], ids: Sequence[str], count, transfer, depth, R: int,
                  clamp_negative: bool = True) -> Tuple[str, str]:
    """``(Felsenstein text, TBE text)``: the tree of a join table with a label after the ``)`` of every join's node."""
    joins, final = table_to_joins(slots, lengths)
    fbp, tbe = labels_of(count, transfer, depth, R)
    return (newick_of_joins(ids, joins, final, clamp_negative, fbp), newick_of_joins(ids, joins, final, clamp_negative, tbe))


# the searches behind the trees of the CLI: suffix of the tree's file -> bme.py's search (None: the NJ tree itself)
SEARCHES = {"nj": None, "bme": "bme_nni", "spr": "bme_spr"}
# the file of a kind's tree with Felsenstein / TBE labels
SUFFIXES = {"nj": ("sup.nwk", "tbe.nwk"), "bme": ("bme.sup.nwk", "bme.tbe.nwk"), "spr": ("spr.sup.nwk", "spr.tbe.nwk")}


def kind_tables(preds: np.ndarray, reps: np.ndarray, n: int, kind: str, with_lengths: bool = False):
    """The Python twins' join tables behind the supports of one file's ``kind`` tree: ``(slots, lengths) [T]`` of the
    file's own tree (``preds [P]``), ``rep_slots int32 [R][T]`` and ``rep_flag bool [R]`` of its replicates' trees
    (``reps [R][P]``), each the NJ table refined by the kind's search.  A replicate with a non-finite distance is flagged
    (its table: zeros); one stopped at the move cap is used as it stands.  The file's own tree with non-finite distances
    has no table: ``(None, None, ...)``.  ``with_lengths``: ``rep_lengths float64 [R][T]`` as a fifth result."""
    from . import bme

    def one(vec):
        dm = bme.matrix_of_preds(vec, n)
        if not np.isfinite(dm).all():
            return None
        joins, final = bme.nj_joins(dm)
        slots = bme.nj_start(dm)
        lengths = np.array([x for _a, _b, la, lb in joins for x in (la, lb)] + list(final[3:]), dtype=np.float64)
        if SEARCHES[kind] is not None:
            slots, lengths, _steps, _length, _status = getattr(bme, SEARCHES[kind])(dm, slots)
        return np.asarray(slots, dtype=np.int32), lengths

    own = one(preds)
    t = 2 * (n - 3) + 3
    rep_slots, rep_flag = np.zeros((len(reps), t), dtype=np.int32), np.zeros(len(reps), dtype=bool)
    rep_lengths = np.zeros((len(reps), t), dtype=np.float64)
    for r, rep in enumerate(reps):
        table = one(rep)
        if table is None:
            rep_flag[r] = True
        else:
            rep_slots[r], rep_lengths[r] = table
    return (own if own is not None else (None, None)) + (rep_slots, rep_flag) + ((rep_lengths,) if with_lengths else ())


def support_newicks(preds: np.ndarray, reps: np.ndarray, ids: Sequence[str], kinds: Sequence[str] = ("nj",),
                    tbe: bool = True, clamp_negative: bool = True) -> Dict[str, str]:
    """The support files of one alignment by the Python twins: ``{suffix: text}`` with, per kind of tree (``"nj"``,
    ``"bme"``, ``"spr"``), ``<kind>.sup.nwk`` (NJ: ``sup.nwk``) - the kind's tree of ``preds [P]`` with Felsenstein labels
    counted over the replicates ``reps [R][P]``, every replicate's NJ tree refined by the same search - and, with
    ``tbe``, ``<kind>.tbe.nwk`` with ``tbe_percent`` labels.  Fewer than four sequences, or non-finite distances of the
    alignment itself: the kind's plain text (no split to support)."""
    from . import bme
    from .bootstrap import support_newick_py
    n = len(ids)
    preds = np.asarray(preds, dtype=np.float32).reshape(-1)
    reps = np.asarray(reps, dtype=np.float32)
    R = reps.shape[0]
    out: Dict[str, str] = {}
    for kind in kinds:
        sup, tb = SUFFIXES[kind]
        slots, lengths, rep_slots, rep_flag = kind_tables(preds, reps, n, kind) if n >= 4 else (None, None, None, None)
        if slots is None:
            plain = {"nj": lambda: support_newick_py(preds, reps, ids, clamp_negative),
                     "bme": lambda: bme.bme_newick_py(preds, ids, clamp_negative),
                     "spr": lambda: bme.spr_newick_py(preds, ids, clamp_negative)}[kind]()
            texts = (plain, plain)
        else:
            texts = support_texts(slots, lengths, ids, *split_supports(slots, rep_slots, n, rep_flag), R, clamp_negative)
        out[sup] = texts[0]
        if tbe:
            out[tb] = texts[1]
    return out
