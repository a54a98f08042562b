"""The arrays of the tree calls - distances, join tables and zeroed results - as ``Engine`` (the device) and ``hostio``
(the same calls without one) both hand them to the library.  numpy only: both modules import it at the top."""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

# results per source of the two families of calls that take distances; a width is a function of T
JOINS = (("slots", np.int32, True), ("lengths", np.float64, True), ("nonfinite", np.uint8, False))
REFINE = (("slots", np.int32, True), ("lengths", np.float64, True), ("steps", np.int32, False),
          ("tree_length", np.float64, False), ("status", np.uint8, False))


def ptr(x: Optional[np.ndarray]):
    """The address of an array for a ``void*`` argument; None (NULL) for no array and for an empty one."""
    return None if x is None or not x.size else x.ctypes.data


def unbatched(out, single: bool):
    """The results of a call whose arguments came without ``B``: without ``B``."""
    return tuple(None if x is None else x[0] for x in out) if single else tuple(out)


def tree_call(preds, family, refuse: Callable, start=None, single_ok: bool = False):
    """Distances ``[B, P]`` (``single_ok``: or ``[P]``) and, for ``REFINE``, start tables ``[B, T]`` (or ``[T]``) →
    ``(preds float32, start int32 or None, (B, N, T), single, zeroed results of family)``.  ``N`` is 0 where ``P`` is no
    number of pairs, ``T = 2 (N - 3) + 3`` and 0 below three sequences.  ``refuse(preds, start, N, T)`` raises what the
    caller does not take, before anything is allocated: the device forms and the host forms differ in that."""
    p = np.ascontiguousarray(np.asarray(preds, dtype=np.float32))
    st = None if start is None else np.ascontiguousarray(np.asarray(start, dtype=np.int32))
    single = single_ok and p.ndim == 1
    if single:
        p = p[None, :]
        st = st[None, :] if st is not None and st.ndim == 1 else st
    pairs = p.shape[1] if p.ndim == 2 else -1
    n = (1 + int(round((1 + 8 * pairs) ** 0.5))) // 2 if pairs >= 0 else 0
    n = n if n * (n - 1) // 2 == pairs else 0
    t = max(0, 2 * (n - 3) + 3)
    refuse(p, st, n, t)
    b = p.shape[0]
    return p, st, (b, n, t), single, tuple(np.zeros((b, t) if wide else b, dtype=dt) for _name, dt, wide in family)


def support_arrays(ref_slots, rep_slots, rep_flag):
    """The arguments of the three ``pf_join_supports`` entry points, checked: ``(ref int32[B, T], rep int32[B, R, T], flag
    uint8[B, R] or None, (B, R, N), single)``."""
    ref = np.ascontiguousarray(np.asarray(ref_slots, dtype=np.int32))
    rep = np.ascontiguousarray(np.asarray(rep_slots, dtype=np.int32))
    single = ref.ndim == 1
    if single:
        ref, rep = ref[None, :], rep[None] if rep.ndim == 2 else rep
    if ref.ndim != 2 or rep.ndim != 3 or rep.shape[0] != ref.shape[0] or rep.shape[2] != ref.shape[1]:
        raise ValueError(f"expected reference tables [B, T] and replicate tables [B, R, T], got {ref.shape} and {rep.shape}")
    b, r, t = rep.shape
    n = (t - 3) // 2 + 3
    if t < 5 or 2 * (n - 3) + 3 != t or b < 1 or r < 1:
        raise ValueError(f"{t} slots are not the join table of N >= 4 sequences, or no source or replicate ({b}, {r})")
    flag = None
    if rep_flag is not None:
        flag = np.ascontiguousarray(np.asarray(rep_flag).astype(bool).astype(np.uint8).reshape(b, r))
    return ref, rep, flag, (b, r, n), single


def support_outputs(b: int, n: int):
    """The results of the three ``pf_join_supports`` entry points, zeroed: ``((count, transfer, depth, status), pointers)``."""
    s = n - 3
    out = (np.zeros((b, s), dtype=np.int32), np.zeros((b, s), dtype=np.int64), np.zeros((b, s), dtype=np.int32),
           np.zeros(b, dtype=np.uint8))
    return out, [ptr(x) for x in out]


def transfer_outputs(b: int, n: int, branch_moves: bool = True):
    """The results of the three ``pf_join_transfers`` entry points, zeroed: ``((count, transfer, depth, moves, used, capped,
    branch_moves or None, status), pointers)``."""
    s = n - 3
    count, transfer, depth, status = support_outputs(b, n)[0]
    out = (count, transfer, depth, np.zeros((b, n), dtype=np.int64), np.zeros((b, s), dtype=np.int32),
           np.zeros((b, s), dtype=np.int32), np.zeros((b, s, n), dtype=np.int32) if branch_moves else None, status)
    return out, [ptr(x) for x in out]


def consensus_arrays(rep_slots, rep_lengths, rep_flag):
    """The arguments of the three ``pf_join_consensus`` entry points, checked: ``(rep int32[B, R, T], lengths float64[B, R,
    T] or None, flag uint8[B, R] or None, (B, R, N), single)``."""
    rep = np.ascontiguousarray(np.asarray(rep_slots, dtype=np.int32))
    single = rep.ndim == 2
    if single:
        rep = rep[None]
    if rep.ndim != 3:
        raise ValueError(f"expected replicate tables [B, R, T] or [R, T], got {rep.shape}")
    b, r, t = rep.shape
    n = (t - 3) // 2 + 3
    if t < 5 or 2 * (n - 3) + 3 != t or b < 1 or r < 1:
        raise ValueError(f"{t} slots are not the join table of N >= 4 sequences, or no source or replicate ({b}, {r})")
    lengths = flag = None
    if rep_lengths is not None:
        lengths = np.ascontiguousarray(np.asarray(rep_lengths, dtype=np.float64).reshape(b, r, t))
    if rep_flag is not None:
        flag = np.ascontiguousarray(np.asarray(rep_flag).astype(bool).astype(np.uint8).reshape(b, r))
    return rep, lengths, flag, (b, r, n), single


def consensus_outputs(b: int, n: int, lengths: bool):
    """The results of a ``pf_join_consensus`` call, zeroed, and their addresses in the order of the C arguments."""
    s = n - 3
    out = (np.zeros(b, dtype=np.int32), np.zeros((b, s), dtype=np.int32), np.zeros((b, s), dtype=np.int32),
           np.zeros((b, s), dtype=np.int32), np.zeros((b, s), dtype=np.float64) if lengths else None,
           np.zeros((b, n), dtype=np.int32), np.zeros((b, n), dtype=np.float64) if lengths else None, np.zeros(b, dtype=np.uint8))
    return out, [ptr(x) for x in out]


def distance_arrays(slots, lengths, flag):
    """The arguments of the three ``pf_join_distances`` entry points, checked: ``(slots int32[B, K, T], lengths float64[B, K,
    T] or None, flag uint8[B, K] or None, (B, K, N), single)``."""
    s = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
    single = s.ndim == 2
    if single:
        s = s[None]
    if s.ndim != 3:
        raise ValueError(f"expected join tables [B, K, T] or [K, T], got {s.shape}")
    b, k, t = s.shape
    n = (t - 3) // 2 + 3
    if t < 5 or 2 * (n - 3) + 3 != t or b < 1 or k < 1:
        raise ValueError(f"{t} slots are not the join table of N >= 4 sequences, or no source or tree ({b}, {k})")
    l = f = None
    if lengths is not None:
        l = np.ascontiguousarray(np.asarray(lengths, dtype=np.float64).reshape(b, k, t))
    if flag is not None:
        f = np.ascontiguousarray(np.asarray(flag).astype(bool).astype(np.uint8).reshape(b, k))
    return s, l, f, (b, k, n), single


def distance_outputs(b: int, k: int, lengths: bool):
    """The results of a ``pf_join_distances`` call, zeroed, and their addresses in the order of the C arguments."""
    out = (np.zeros((b, k, k), dtype=np.int32), np.zeros((b, k, k), dtype=np.float64) if lengths else None,
           np.zeros((b, k, k), dtype=np.float64) if lengths else None, np.zeros(b, dtype=np.uint8))
    return out, [ptr(x) for x in out]
