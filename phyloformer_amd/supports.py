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
from .nj import join_splits, newick_of_joins, table_of_joins
from .treekinds import NJ_STARTED

# From this many sequences on the CLI matches a sub-batch's supports on the GPU thread (``Engine.join_supports``)
# instead of on the writer threads' serial twin.  A measured constant by ``bme.BME_DEVICE_MIN``'s rule (DESIGN.md
# section 23, tools/support_bench.py, profiles/support_bench.txt): the smallest measured N at which the device side
# takes at most half the host's time at R = 100; None = the device path is off in the CLI (the API stays).
SUPPORT_DEVICE_MIN = 200

# From this many sequences on the CLI's ``--instability`` counts a sub-batch's transfers on the GPU thread
# (``Engine.join_transfers``) instead of on the writer threads' serial twin.  The same rule (DESIGN.md section 27,
# tools/support_bench.py --transfers, profiles/transfer_bench.txt: 36 times the host's speed at N = 200, 1.5 times at 50);
# None = the device path is off in the CLI.
TRANSFER_DEVICE_MIN = 200


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


def transfer_taxa(ref_slots: Sequence[int], rep_slots: Sequence[Sequence[int]], n: int,
                  rep_flag: Optional[Sequence[bool]] = None, cutoff: int = 100) -> Dict[str, list]:
    """One source: which sequences have to move (the per-taxon companion of the transfer bootstrap,
    Lemoine et al. 2018).  For reference split ``s`` (join ``t``, depth ``p``) and an unflagged replicate with splits
    ``q_j`` in join order, ``m_j = min(h_j, n - h_j)`` and ``side_j = 0`` if ``h_j <= n - h_j`` else 1; ``j*`` has the least
    ``(m_j, j)`` and ``delta = min(p - 1, m_j*)`` as in ``split_supports``.  If ``m_j* <= p - 1`` the transfer set is
    ``X = s xor q_j*``, complemented within the ``n`` sequences if ``side_j* = 1`` (``popcount(X) = delta``); otherwise,
    or if the replicate is flagged, the pair is *capped*: the leaf edges give ``p - 1`` and nothing is attributed to any
    sequence.  The pair is *used* iff ``100 delta <= cutoff (p - 1)``, ``cutoff`` an integer percent.

    Returns ``{"count", "transfer", "depth"}`` as ``split_supports`` and ``"used"[t]`` = used replicates, ``"capped"[t]``
    = used replicates that are capped, ``"branch_moves"[t][x]`` = used, uncapped replicates with ``x`` in ``X``,
    ``"moves"[x]`` = the sum of ``branch_moves[t][x]`` over ``t``.  At ``cutoff = 100`` every pair is used and
    ``sum_x branch_moves[t][x] + (p_t - 1) capped[t] == transfer[t]``."""
    cutoff = int(cutoff)
    if not 0 <= cutoff <= 100:
        raise ValueError(f"the cutoff is a percent from 0 to 100 (got {cutoff})")
    if len(rep_slots) < 1:
        raise ValueError("split supports need R >= 1 replicates")
    flags = [False] * len(rep_slots) if rep_flag is None else [bool(f) for f in rep_flag]
    if len(flags) != len(rep_slots):
        raise ValueError(f"expected {len(rep_slots)} replicate flags, got {len(flags)}")
    ref = table_splits(ref_slots, n)
    reps = [None if f else table_splits(s, n) for s, f in zip(rep_slots, flags)]
    everyone = (1 << n) - 1
    out = {k: [] for k in ("count", "transfer", "depth", "used", "capped", "branch_moves")}
    out["moves"] = [0] * n
    for s in ref:
        k = bin(s).count("1")
        p = min(k, n - k)
        c = total = used = capped = 0
        row = [0] * n
        for splits in reps:
            best = None                                          # (m, j, side) of the closest split
            for j, q in enumerate(splits or ()):
                h = bin(s ^ q).count("1")
                key = (min(h, n - h), j, 0 if h <= n - h else 1)
                if best is None or key < best:
                    best = key
            is_capped = best is None or best[0] > p - 1
            delta = p - 1 if is_capped else best[0]
            c += delta == 0
            total += delta
            if 100 * delta > cutoff * (p - 1):
                continue
            used += 1
            if is_capped:
                capped += 1
                continue
            X = s ^ splits[best[1]]
            if best[2]:
                X ^= everyone
            for x in range(n):
                row[x] += (X >> x) & 1
        for name, v in (("count", c), ("transfer", total), ("depth", p), ("used", used), ("capped", capped), ("branch_moves", row)):
            out[name].append(v)
        out["moves"] = [a + b for a, b in zip(out["moves"], row)]
    return out


def instability_permille(moves: int, used: int) -> int:
    """``moves / used`` in permille, rounded half up: how often, per used (reference branch, replicate) pair, the
    sequence is among those that have to move.  0 where no pair is used."""
    moves, used = int(moves), int(used)
    return (2000 * moves + used) // (2 * used) if used else 0


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


# the files of --instability per kind of tree: per-taxon counts, per-branch counts, the tree labelled with the join t
INSTABILITY_SUFFIXES = {k.name: k.files("instability.tsv", "branches.tsv", "branches.nwk") for k in NJ_STARTED}
TOP_MOVED = 5


def instability_texts(slots: Optional[Sequence[int]], lengths, ids: Sequence[str], res, R: int, plain: str = "",
                      clamp_negative: bool = True) -> Tuple[str, str, str]:
    """The three files of ``--instability`` for one tree: ``res`` = ``(count, transfer, depth, moves, used, capped,
    branch_moves)`` of one source (``transfer_taxa``'s or a native entry point's).
    ``instability.tsv``: ``id``, ``moves``, ``permille`` (``instability_permille`` over the tree's used pairs), in input
    order.  ``branches.tsv``: per join ``t`` its ``depth``, Felsenstein percent, TBE percent, ``used``, ``capped`` and
    the (at most) ``TOP_MOVED`` most-moved sequences as ``id:count``, ties in input order, ``-`` if none moved.
    ``branches.nwk``: the tree with ``t`` after the ``)`` of join ``t``'s node.  A tree without a split (``slots`` None:
    fewer than four sequences, or non-finite distances): zeros, no branch, and the ``plain`` text."""
    head = "id\tmoves\tpermille\n"
    cols = "t\tdepth\tsupport\ttbe\tused\tcapped\tmost_moved\n"
    if slots is None:
        return head + "".join(f"{i}\t0\t0\n" for i in ids), cols, plain
    count, transfer, depth, moves, used, capped, branch_moves = ([int(v) for v in x] if k != 6 else x for k, x in enumerate(res[:7]))
    total = sum(used)
    taxa = head + "".join(f"{i}\t{m}\t{instability_permille(m, total)}\n" for i, m in zip(ids, moves))
    fbp, tbe = labels_of(count, transfer, depth, R)
    rows = []
    for t in range(len(count)):
        row = [int(v) for v in branch_moves[t]]
        top = sorted((x for x in range(len(row)) if row[x] > 0), key=lambda x: (-row[x], x))[:TOP_MOVED]
        rows.append(f"{t}\t{depth[t]}\t{fbp[t]}\t{tbe[t]}\t{used[t]}\t{capped[t]}\t" +
                    (",".join(f"{ids[x]}:{row[x]}" for x in top) or "-") + "\n")
    joins, final = table_to_joins(slots, lengths)
    return taxa, cols + "".join(rows), newick_of_joins(ids, joins, final, clamp_negative, list(range(len(count))))


def transfer_tuple(out: Dict[str, list]) -> tuple:
    """``transfer_taxa``'s dict in the order of the native entry points' results (without ``status``)."""
    return tuple(out[k] for k in ("count", "transfer", "depth", "moves", "used", "capped", "branch_moves"))


# the searches behind the trees of the CLI: suffix of the tree's file -> bme.py's search (None: the NJ tree itself)
SEARCHES = {k.name: k.search for k in NJ_STARTED}
# the file of a kind's tree with Felsenstein / TBE labels
SUFFIXES = {k.name: k.files("sup.nwk", "tbe.nwk") for k in NJ_STARTED}


def joins_py(start: str, preds: np.ndarray):
    """``Engine.nj_joins`` (``start`` "nj") / ``Engine.bionj_joins`` ("bionj") by the statements: ``float32 [M, P_N]`` ->
    ``(slots int32 [M, T], lengths float64 [M, T], nonfinite bool [M])``; a flagged source's table is zeros."""
    from . import bionj, bme
    preds = np.asarray(preds, dtype=np.float32)
    n = (1 + int(round((1 + 8 * preds.shape[1]) ** 0.5))) // 2
    slots = np.zeros((len(preds), 2 * n - 3), dtype=np.int32)
    lengths = np.zeros((len(preds), 2 * n - 3), dtype=np.float64)
    bad = np.zeros(len(preds), dtype=bool)
    for m, vec in enumerate(preds):
        dm = bme.matrix_of_preds(vec, n)
        bad[m] = not np.isfinite(dm).all()
        if not bad[m]:
            slots[m], lengths[m] = table_of_joins(*(bme.nj_joins if start == "nj" else bionj.bionj_joins)(dm))
    return slots, lengths, bad


def refine_py(search: str, preds: np.ndarray, start_slots: np.ndarray):
    """``Engine.bme_nni`` / ``Engine.bme_spr`` by the statements (``bme.py``'s function of that name, source by source):
    ``(slots [M, T], lengths [M, T], steps [M], tree_length [M], status [M])``."""
    from . import bme
    preds = np.asarray(preds, dtype=np.float32)
    n = (1 + int(round((1 + 8 * preds.shape[1]) ** 0.5))) // 2
    out = [getattr(bme, search)(bme.matrix_of_preds(vec, n), start) for vec, start in zip(preds, start_slots)]
    return tuple(np.array(x) for x in zip(*out))


def kind_tables(preds: np.ndarray, reps: np.ndarray, n: int, kind: str, with_lengths: bool = False):
    """The Python twins' join tables behind the supports of one file's ``kind`` tree: ``(slots, lengths) [T]`` of the
    file's own tree (``preds [P]``), ``rep_slots int32 [R][T]`` and ``rep_flag bool [R]`` of its replicates' trees
    (``reps [R][P]``), each the NJ table refined by the kind's search (``treekinds.join_refine`` on the statements).  A
    replicate with a non-finite distance is flagged (its table: zeros); one stopped at the move cap is used as it stands.
    The file's own tree with non-finite distances has no table: ``(None, None, ...)``.  ``with_lengths``: ``rep_lengths
    float64 [R][T]`` as a fifth result."""
    from .treekinds import PythonHost, join_refine
    every = np.concatenate([np.asarray(preds, dtype=np.float32).reshape(1, -1), np.asarray(reps, dtype=np.float32)])
    search = SEARCHES[kind]
    slots, lengths, _steps, bad = join_refine(PythonHost(), "nj", [search] if search else [], every)[search]
    own = (None, None) if bad[0] else (slots[0], lengths[0])
    return own + (slots[1:], bad[1:]) + ((lengths[1:],) if with_lengths else ())


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
