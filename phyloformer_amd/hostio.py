"""ctypes bindings of the native file-format helpers (``csrc/pf_hostio.cpp``).

Same results and the same exception types as the pure-Python mirrors of the
reference in :mod:`fasta` (``load_alignment``, /root/reference/phyloformer/data.py:11-31)
and :mod:`phylip` (``vec_to_phylip``, /root/reference/infer_alns.py:14-25), ~10x
faster and with the GIL released, so the CLI's loader and writer threads run
beside the GPU instead of in front of it.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Sequence, Tuple

import numpy as np

from .cabi import CONSTANTS
from .engine import load_library
from .treearrays import (JOINS, REFINE, consensus_arrays, consensus_outputs, distance_arrays, distance_outputs, ptr, support_arrays, support_outputs,
                         transfer_outputs, tree_call, unbatched)

# library functions of this module that are not part of include/phyloformer_amd.h (bound here, not in
# engine.SIGNATURES, whose set must equal the header's)
_PRIVATE = {
    "pf_nj_support_n": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p,
                                    C.c_int32, C.c_int32, C.c_char_p, C.c_int64]),
    "pf_bme_newick_steps_n": (C.c_int64, [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_int32, C.c_char_p,
                                          C.c_int64, C.c_void_p]),
    "pf_bme_spr_newick_steps_n": (C.c_int64, [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_int32, C.c_char_p,
                                              C.c_int64, C.c_void_p]),
    "pf_nj_joins_host_n": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
}


_bound = None


def _lib():
    global _bound
    lib = load_library()
    if lib is not _bound:
        for name, (res, args) in _PRIVATE.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _bound = lib
    return lib


# pf_parse_fasta's codes and pf_status' PF_EIO, as include/phyloformer_amd.h defines them
PF_FASTA_EBYTE, PF_FASTA_ERAGGED, PF_FASTA_ENOHEADER, PF_FASTA_EEMPTY, PF_FASTA_ECAP, PF_FASTA_EUTF8, PF_EIO = (
    CONSTANTS[k] for k in ("PF_FASTA_EBYTE", "PF_FASTA_ERAGGED", "PF_FASTA_ENOHEADER", "PF_FASTA_EEMPTY", "PF_FASTA_ECAP",
                           "PF_FASTA_EUTF8", "PF_EIO"))


def parse_error(rc: int, l: int, detail: int, path: str = "", data: bytes = b"") -> "BaseException | None":
    """The exception the reference raises where pf_parse_fasta returns ``rc`` (None = a valid alignment)."""
    if rc == PF_FASTA_EUTF8:
        # the header at offset `detail` is not UTF-8: let bytes.decode build the reference's exception (data.py:22)
        if not data and path:
            with open(path, "rb") as fh:
                data = fh.read()
        line = data[int(detail):].split(b"\n", 1)[0].strip()
        try:
            line.decode("utf8")
        except UnicodeDecodeError as exc:
            return exc
        return UnicodeDecodeError("utf-8", line, 0, 1, "invalid header")
    if rc == PF_FASTA_EBYTE:
        return KeyError(int(detail))
    if rc == PF_FASTA_ENOHEADER:
        return IndexError("sequence data before the first '>' header")
    if rc == PF_FASTA_EEMPTY or (rc == 0 and l == 0):
        # same class as the reference, whose one_hot refuses the empty tensor (data.py:28)
        return RuntimeError("no residues found (empty alignment)")
    if rc == PF_FASTA_ERAGGED:
        return ValueError("expected sequences of equal length")
    if rc == PF_EIO:
        import os
        return OSError(int(detail), os.strerror(int(detail)), path)
    if rc != 0:
        return RuntimeError(f"pf_parse_fasta failed with status {rc}")
    return None


def parse_fasta(data: bytes) -> Tuple[np.ndarray, List[str]]:
    """FASTA bytes → ``(uint8[N, L] residue indices, ids)``."""
    lib = load_library()
    n_max = data.count(b">") + 1
    idx = np.empty(len(data), dtype=np.uint8)
    spans = np.empty(2 * n_max, dtype=np.int64)
    n, l, detail = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    rc = lib.pf_parse_fasta(data, len(data), idx.ctypes.data, idx.size, spans.ctypes.data, n_max,
                            C.byref(n), C.byref(l), C.byref(detail))
    exc = parse_error(rc, l.value, detail.value, data=data)
    if exc is not None:
        raise exc
    ids = [data[int(spans[2 * i]):int(spans[2 * i] + spans[2 * i + 1])].decode("utf8") for i in range(n.value)]
    return idx[:n.value * l.value].reshape(n.value, l.value).copy(), ids


def load_alignment(filepath) -> Tuple[np.ndarray, List[str]]:
    with open(filepath, "rb") as fh:
        return parse_fasta(fh.read())


def _ids(ids: Sequence[str]):
    """ids → ``(c_char_p array, int64 byte lengths, the encoded ids)``.  Explicit lengths: an id may hold NUL bytes.  The
    encoded list must stay referenced during the call."""
    enc = [s.encode("utf8") for s in ids]
    return (C.c_char_p * len(enc))(*enc), np.array([len(e) for e in enc], dtype=np.int64), enc


def _pair_vector(preds, n: int) -> np.ndarray:
    """The distances of ``n`` sequences as a contiguous float32 vector ``[n (n - 1) / 2]``."""
    p = np.ascontiguousarray(np.asarray(preds, dtype=np.float32).reshape(-1))
    if p.size != n * (n - 1) // 2:
        raise ValueError(f"expected {n * (n - 1) // 2} distances for {n} sequences, got {p.shape}")
    return p


def _check_rc(symbol: str, rc: int, hint: str = ""):
    """The status of a host call: ``-1`` of a call with a ``hint`` of what it refuses is a ``ValueError``, every other
    negative code a ``RuntimeError``."""
    if rc == -1 and hint:
        raise ValueError(f"{symbol} refused its arguments ({hint}?)")
    if rc < 0:
        raise RuntimeError(f"{symbol} failed with status {rc}")


def _text_call(symbol: str, lead, trail, cap: int, retry: bool = True, name: str = "") -> bytes:
    """The sizing protocol of a text call ``symbol(*lead, out, cap, *trail)`` → the text's size: one call with a buffer of
    ``cap`` bytes (0: none, a query) and, where the text is longer, ``retry`` with the size it returned.  ``name``: what
    the error calls the function, where that is not ``symbol``."""
    fn = getattr(_lib(), symbol)
    buf = C.create_string_buffer(cap) if cap else None
    w = fn(*lead, buf, cap, *trail)
    if retry and w > cap:
        cap = int(w)
        buf = C.create_string_buffer(cap)
        w = fn(*lead, buf, cap, *trail)
    if w < 0 or w > cap:
        raise RuntimeError(f"{name or symbol} failed with status {w}")
    return buf.raw[:w] if buf is not None else b""


def _newick_call(symbol: str, preds, ids: Sequence[str], clamp_negative: bool, guess: bool, trail=(), name: str = "") -> bytes:
    """A text call on distances ``[P]`` + ids.  ``guess``: the first buffer has room for the NJ text with longer numbers
    (one run of an expensive call, not two); else the call is queried first."""
    n = len(ids)
    p = _pair_vector(preds, n)
    arr, lens, _enc = _ids(ids)
    cap = int(lens.sum()) + 64 * max(n, 1) + 64 if guess else 0
    return _text_call(symbol, (p.ctypes.data, n, arr, lens.ctypes.data, int(clamp_negative)), trail, cap, name=name)


def format_phylip(preds: np.ndarray, ids: Sequence[str]) -> bytes:
    """Distance vector ``[P]`` + ids → PHYLIP text (utf-8 bytes), byte-identical to ``vec_to_phylip``."""
    n = len(ids)
    p = _pair_vector(preds, n)
    arr, lens, _enc = _ids(ids)
    cap = int(lens.sum()) + n * (n * 24 + 2) + 32                # (longer only with astronomically large distances)
    return _text_call("pf_format_phylip_n", (p.ctypes.data, n, arr, lens.ctypes.data), (), cap, name="pf_format_phylip")


def nj_newick(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> bytes:
    """Distance vector ``[P]`` + ids → Newick text of the neighbour-joining tree (utf-8 bytes), byte-identical to
    ``nj.neighbor_joining`` on the matrix ``vec_to_phylip`` builds (the CLI's ``--trees``, infer_alns.py:120-123)."""
    return _newick_call("pf_nj_newick_n", preds, ids, clamp_negative, guess=False)


def bionj_newick(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> bytes:
    """``pf_bionj_newick_n``: distance vector ``[P]`` + ids → Newick text (utf-8 bytes) of the BIONJ tree (the CLI's
    ``--bionj``) - byte-identical to ``bionj.bionj_newick_py``."""
    return _newick_call("pf_bionj_newick_n", preds, ids, clamp_negative, guess=True)


def bionj_refined_newick(search: str, preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> bytes:
    """``<stem>.bionj.bme.nwk`` / ``<stem>.bionj.spr.nwk`` (``search`` = ``"bme"`` / ``"spr"``): ``pf_bionj_joins_host`` →
    ``pf_bme_nni_host`` / ``pf_bme_spr_host`` → ``pf_nj_format_joins_n`` - byte-identical to
    ``bionj.bionj_bme_newick_py`` / ``bionj.bionj_spr_newick_py``.  Fewer than three sequences or non-finite distances:
    the NJ text."""
    n = len(ids)
    p = np.ascontiguousarray(np.asarray(preds, dtype=np.float32).reshape(-1))
    if n < 3 or not np.isfinite(p).all():
        return nj_newick(p, ids, clamp_negative)
    start, _lengths, _flag = bionj_joins_host(p[None, :])
    slots, lengths, _steps, _length, _status = (bme_nni_host if search == "bme" else bme_spr_host)(p[None, :], start)
    return newick_of_joins(slots[0], lengths[0], ids, clamp_negative)


def bme_newick(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True, with_steps: bool = False):
    """``pf_bme_newick_n``: distance vector ``[P]`` + ids → Newick text (utf-8 bytes) of the neighbour-joining tree refined
    by balanced NNIs, with balanced branch lengths (the CLI's ``--bme``) - byte-identical to ``bme.bme_newick_py``.
    ``with_steps``: ``(text, moves)``."""
    return _refined_newick("pf_bme_newick", preds, ids, clamp_negative, with_steps)


def spr_newick(preds: np.ndarray, ids: Sequence[str], clamp_negative: bool = True, with_steps: bool = False):
    """``pf_bme_spr_newick_n``: as ``bme_newick``, the tree refined by balanced SPR moves (the CLI's ``--spr``) -
    byte-identical to ``bme.spr_newick_py``."""
    return _refined_newick("pf_bme_spr_newick", preds, ids, clamp_negative, with_steps)


def _refined_newick(stem: str, preds: np.ndarray, ids: Sequence[str], clamp_negative: bool, with_steps: bool):
    steps = C.c_int32(0)
    text = _newick_call(stem + "_steps_n", preds, ids, clamp_negative, guess=True, trail=(C.byref(steps),), name=stem + "_n")
    return (text, int(steps.value)) if with_steps else text


def _refuse_refine(p, st, n, t):
    if p.ndim != 2 or st.ndim != 2 or st.shape[0] != p.shape[0]:
        raise ValueError(f"expected distances [B, P] and start tables [B, T], got {p.shape} and {st.shape}")
    if n < 3 or st.shape[1] != t or p.shape[0] < 1:
        raise ValueError(f"{p.shape[1]} distances and {st.shape[1]} slots are not those of N >= 3 sequences")


def _refuse_joins(p, _st, n, _t):
    if p.ndim != 2 or p.shape[0] < 1:
        raise ValueError(f"expected distances [B >= 1, P], got {p.shape}")
    if n < 3:
        raise ValueError(f"{p.shape[1]} distances are not the pairs of N >= 3 sequences")


def bme_nni_host(preds: np.ndarray, start_slots: np.ndarray):
    """``pf_bme_nni_host``: ``Engine.bme_nni`` without a device - the same bodies run serially, the same bits.
    ``float32[B, P_N]``, ``int32[B, T]`` → ``(slots, lengths, steps, tree_length, status)``.  ``ValueError`` for what
    the library refuses (``N < 3``, an invalid start table)."""
    return _refine_host("pf_bme_nni_host", preds, start_slots)


def bme_spr_host(preds: np.ndarray, start_slots: np.ndarray):
    """``pf_bme_spr_host``: ``Engine.bme_spr`` without a device, as ``bme_nni_host`` is ``Engine.bme_nni``'s."""
    return _refine_host("pf_bme_spr_host", preds, start_slots)


def _refine_host(symbol: str, preds: np.ndarray, start_slots: np.ndarray):
    p, st, (b, n, _t), _single, out = tree_call(preds, REFINE, _refuse_refine, start_slots)
    _check_rc(symbol, getattr(_lib(), symbol)(p.ctypes.data, st.ctypes.data, b, n, *map(ptr, out)), "an invalid start table")
    return out


def nj_joins_host(preds: np.ndarray, threads: int = 1):
    """``Engine.nj_joins`` without a device (``pf_nj_joins_host_n``): ``float32[B, P_N]`` → ``(slots int32[B, T], lengths
    float64[B, T], nonfinite bool[B])``, the table of ``nj.nj_joins`` bit for bit; a flagged source's table is zeros."""
    return _joins_host("pf_nj_joins_host_n", preds, int(threads))


def bionj_joins_host(preds: np.ndarray):
    """``Engine.bionj_joins`` without a device (``pf_bionj_joins_host``): ``float32[B, P_N]`` → ``(slots int32[B, T],
    lengths float64[B, T], nonfinite bool[B])``, the table of ``bionj.bionj_joins`` bit for bit; a flagged source's
    table is zeros.  ``RuntimeError`` for what the library refuses."""
    return _joins_host("pf_bionj_joins_host", preds)


def delta_host(preds: np.ndarray, n: int = 0, bins: int = 20):
    """``Engine.delta`` without a device (``pf_delta_host``): ``float32[B, P_n]`` (or ``[P_n]``; ``n`` = 0 takes it from
    the width) → ``(pair_sum int64[B, P_n], hist int64[B, bins], nonfinite uint8[B])``, every quartet visited once,
    serially: ``delta.delta_py`` bit for bit.  ``ValueError`` for what the library refuses."""
    from .delta import delta_arrays
    p, (b, n), single, out = delta_arrays(preds, bins, n)
    _check_rc("pf_delta_host", _lib().pf_delta_host(ptr(p), b, n, int(bins), *map(ptr, out)), "N, B or K out of range")
    return unbatched(out, single)


def tree_fit_host(preds: np.ndarray, slots: np.ndarray, lengths: np.ndarray, patristic: bool = True):
    """``Engine.tree_fit`` without a device (``pf_tree_fit_host``), its arguments and results: every tree of every source
    serially, ``fit.tree_fit_py`` bit for bit.  ``ValueError`` for what the library refuses."""
    from .fit import fit_arrays, squeezed
    p, s, l, (b, m, n), flags, out = fit_arrays(preds, slots, lengths, patristic)
    _check_rc("pf_tree_fit_host", _lib().pf_tree_fit_host(ptr(p), ptr(s), ptr(l), b, m, n, *map(ptr, out)), "N, B or M out of range")
    return squeezed(out, flags)


def tree_ols_host(preds: np.ndarray, slots: np.ndarray):
    """``Engine.tree_ols`` without a device (``pf_tree_ols_host``), its arguments and results: every tree of every source
    serially, ``ols.tree_ols_py`` bit for bit.  ``ValueError`` for what the library refuses."""
    from .ols import ols_arrays, squeezed
    p, s, (b, m, n), flags, out = ols_arrays(preds, slots)
    _check_rc("pf_tree_ols_host", _lib().pf_tree_ols_host(ptr(p), ptr(s), b, m, n, *map(ptr, out)), "N, B or M out of range")
    return squeezed(out, flags)


def tree_root_host(slots: np.ndarray, lengths: np.ndarray):
    """``Engine.tree_root`` without a device (``pf_tree_root_host``), its arguments and results: every tree serially,
    ``root.tree_root_py`` bit for bit.  ``ValueError`` for what the library refuses."""
    from .root import root_arrays, squeezed
    s, l, (b, m, n), flags, out = root_arrays(slots, lengths)
    _check_rc("pf_tree_root_host", _lib().pf_tree_root_host(ptr(s), ptr(l), b, m, n, *map(ptr, out)), "N, B or M out of range")
    return squeezed(out, flags)


def _joins_host(symbol: str, preds: np.ndarray, *options):
    p, _, (b, n, _t), _single, (slots, lengths, flag) = tree_call(preds, JOINS, _refuse_joins)
    _check_rc(symbol, getattr(_lib(), symbol)(p.ctypes.data, b, n, *options, ptr(slots), ptr(lengths), ptr(flag)))
    return slots, lengths, flag.astype(bool)


def join_supports_host(ref_slots, rep_slots, rep_flag=None):
    """``pf_join_supports_host``: ``Engine.join_supports`` without a device - the same bodies run serially, the same
    integers as ``supports.split_supports``.  ``ValueError`` for what the library refuses (``N < 4``, a table that is no
    join table)."""
    ref, rep, flag, (b, r, n), single = support_arrays(ref_slots, rep_slots, rep_flag)
    out, ptrs = support_outputs(b, n)
    _check_rc("pf_join_supports_host", _lib().pf_join_supports_host(ref.ctypes.data, rep.ctypes.data, ptr(flag), b, r, n, *ptrs),
              "a table that is no join table")
    return unbatched(out, single)


def join_transfers_host(ref_slots, rep_slots, rep_flag=None, cutoff: int = 100, branch_moves: bool = True):
    """``pf_join_transfers_host``: ``Engine.join_transfers`` without a device - the same bodies run serially, the same
    integers as ``supports.transfer_taxa``.  ``ValueError`` for what the library refuses (``N < 4``, a table that is no
    join table, a cutoff outside 0 .. 100)."""
    ref, rep, flag, (b, r, n), single = support_arrays(ref_slots, rep_slots, rep_flag)
    out, ptrs = transfer_outputs(b, n, branch_moves)
    _check_rc("pf_join_transfers_host",
              _lib().pf_join_transfers_host(ref.ctypes.data, rep.ctypes.data, ptr(flag), b, r, n, int(cutoff), *ptrs),
              "a table that is no join table, a cutoff outside 0 .. 100")
    return unbatched(out, single)


def join_consensus_host(rep_slots, rep_lengths=None, rep_flag=None, percent: int = 50):
    """``pf_join_consensus_host``: ``Engine.join_consensus`` without a device - the same bodies run serially, the integers
    and (bit for bit) the doubles of ``consensus.join_consensus``; a source with a table that is no join table comes back
    with status 1 and zeros.  ``ValueError`` for what the library refuses (``N < 4``, a threshold outside 50 .. 99)."""
    rep, lengths, flag, (b, r, n), single = consensus_arrays(rep_slots, rep_lengths, rep_flag)
    out, ptrs = consensus_outputs(b, n, lengths is not None)
    _check_rc("pf_join_consensus_host",
              _lib().pf_join_consensus_host(rep.ctypes.data, ptr(lengths), ptr(flag), b, r, n, int(percent), *ptrs),
              f"a threshold of {percent} percent outside 50 .. 99")
    return unbatched(out, single)


def join_distances_host(slots, lengths=None, flag=None):
    """``pf_join_distances_host``: ``Engine.join_distances`` without a device - the same bodies run serially, the integers
    and (bit for bit) the doubles of ``treedist.join_distances_py``; a source with a table that is no join table comes back
    with status 1 and zeros.  ``ValueError`` for what the library refuses (``N < 4``, ``K > 4096``)."""
    s, l, f, (b, k, n), single = distance_arrays(slots, lengths, flag)
    out, ptrs = distance_outputs(b, k, l is not None)
    _check_rc("pf_join_distances_host", _lib().pf_join_distances_host(s.ctypes.data, ptr(l), ptr(f), b, k, n, *ptrs),
              f"K = {k} trees or N = {n} sequences out of range")
    return unbatched(out, single)


def _join_table(slots, lengths, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """One source's join table (``Engine.nj_joins``) for ``n`` ids, checked: ``2 (n - 3) + 3`` slots in ``[0, n)``."""
    s = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
    l = np.ascontiguousarray(np.asarray(lengths, dtype=np.float64).reshape(-1))
    t = 2 * (n - 3) + 3
    if n < 3 or s.size != t or l.size != t:
        raise ValueError(f"expected a join table of {max(t, 0)} entries for {n} >= 3 sequences, got {s.size} slots and {l.size} lengths")
    if s.size and (int(s.min()) < 0 or int(s.max()) >= n):
        raise ValueError(f"join table names a slot outside [0, {n})")
    return s, l


def newick_of_joins(slots, lengths, ids: Sequence[str], clamp_negative: bool = True) -> bytes:
    """``pf_nj_format_joins_n``: the Newick text (utf-8 bytes) of one source's join table - ``Engine.nj_joins``'s ``slots``
    / ``lengths [2 (n - 3) + 3]`` - byte-identical to ``nj.newick_of_joins``; with the table of the same distances it is
    ``nj_newick``'s text."""
    n = len(ids)
    s, l = _join_table(slots, lengths, n)
    arr, lens, _enc = _ids(ids)
    return _text_call("pf_nj_format_joins_n", (s.ctypes.data, l.ctypes.data, n, arr, lens.ctypes.data, int(clamp_negative)), (), 0)


def newick_of_joins_py(slots, lengths, ids: Sequence[str], clamp_negative: bool = True) -> str:
    """The pure-Python equivalent of ``newick_of_joins``: the table handed to ``nj.newick_of_joins``."""
    from .nj import newick_of_joins as text_of
    n = len(ids)
    s, l = _join_table(slots, lengths, n)
    j = n - 3
    joins = [(int(s[2 * t]), int(s[2 * t + 1]), float(l[2 * t]), float(l[2 * t + 1])) for t in range(j)]
    final = (int(s[2 * j]), int(s[2 * j + 1]), int(s[2 * j + 2]), float(l[2 * j]), float(l[2 * j + 1]), float(l[2 * j + 2]))
    return text_of(ids, joins, final, clamp_negative)


def nj_support(preds: np.ndarray, reps: np.ndarray, ids: Sequence[str], clamp_negative: bool = True,
               threads: int = 1) -> bytes:
    """``pf_nj_support_n``: the ``nj_newick`` text of ``preds [P]`` with the bootstrap support of every internal node,
    counted over the NJ trees of ``reps [R][P]`` (joined on ``threads`` native threads, GIL released) - byte-identical
    to ``bootstrap.support_newick_py``."""
    n = len(ids)
    p = _pair_vector(preds, n)
    r = np.ascontiguousarray(np.asarray(reps, dtype=np.float32))
    if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] != p.size:
        raise ValueError(f"expected replicates [R >= 1][{p.size}], got {r.shape}")
    arr, lens, _enc = _ids(ids)
    # one NJ sizes the text: the labels add at most "100" per internal node.  Every call joins all replicates: no retry
    base = _lib().pf_nj_newick_n(p.ctypes.data, n, arr, lens.ctypes.data, int(clamp_negative), None, 0)
    _check_rc("pf_nj_newick_n", base)
    return _text_call("pf_nj_support_n", (p.ctypes.data, r.ctypes.data, r.shape[0], n, arr, lens.ctypes.data, int(clamp_negative),
                                          int(threads)), (), int(base) + 3 * n + 16, retry=False)


class FastaBatch:
    """``pf_fasta_batch_load``: a list of FASTA files read and parsed on native threads (GIL released for the
    whole call).  The parsed alignments stay in library memory; ``gather`` copies the residue indices of a
    same-shaped selection into one ``uint8[B, N, L]`` array and ``write_phylip`` formats and writes their
    distance matrices with the ids the batch holds - Python never touches residues or ids on that path."""

    def __init__(self, paths: Sequence[str], threads: int = 8):
        self._lib = load_library()
        self.paths = list(paths)
        self._h = C.c_void_p()
        enc = [os.fsencode(p) for p in self.paths]
        arr = (C.c_char_p * len(enc))(*enc)
        rc = self._lib.pf_fasta_batch_load(arr, len(enc), int(threads), C.byref(self._h))
        if rc != 0:
            raise MemoryError("pf_fasta_batch_load failed") if rc == -4 else RuntimeError(f"pf_fasta_batch_load: status {rc}")
        k = len(enc)
        self.status = np.empty(k, np.int32)
        self.n = np.empty(k, np.int32)
        self.l = np.empty(k, np.int32)
        self.detail = np.empty(k, np.int64)
        self._lib.pf_fasta_batch_infos(self._h, self.status.ctypes.data, self.n.ctypes.data, self.l.ctypes.data,
                                       self.detail.ctypes.data)

    def __len__(self):
        return len(self.paths)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pf_fasta_batch_free(self._h)
            self._h = None

    __del__ = close

    def error(self, i: int) -> "BaseException | None":
        """What ``load_alignment`` raises for file ``i`` (None: a valid alignment)."""
        return parse_error(int(self.status[i]), int(self.l[i]), int(self.detail[i]), self.paths[i])

    def ids(self, i: int) -> List[str]:
        out, p, ln = [], C.c_void_p(), C.c_int64()
        for s in range(int(self.n[i])):
            if self._lib.pf_fasta_batch_id(self._h, i, s, C.byref(p), C.byref(ln)) != 0:
                raise IndexError((i, s))
            out.append(C.string_at(p, ln.value).decode("utf8"))
        return out

    def indices(self, i: int) -> np.ndarray:
        return gather([(self, i)], int(self.n[i]), int(self.l[i]))[0]


def gather(entries: Sequence[Tuple["FastaBatch", int]], n: int, l: int) -> np.ndarray:
    """``uint8[B, N, L]`` of the ``(batch, file)`` entries, all of shape ``(n, l)``."""
    lib = load_library()
    k = len(entries)
    hs = (C.c_void_p * k)(*[e[0]._h for e in entries])
    fi = np.array([e[1] for e in entries], dtype=np.int32)
    out = np.empty((k, n, l), dtype=np.uint8)
    rc = lib.pf_fasta_batch_gather(hs, fi.ctypes.data, k, n, l, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"pf_fasta_batch_gather: status {rc} (entries of another shape than {n} x {l}?)")
    return out


def write_phylip(entries: Sequence[Tuple["FastaBatch", int]], n: int, preds: np.ndarray, out_paths: Sequence[str],
                 threads: int = 8, tree_paths: "Sequence[str] | None" = None) -> None:
    """Format ``preds[B, P]`` and write ``out_paths`` - and, with ``tree_paths``, the neighbour-joining trees of the same
    distances - on native threads; ``OSError`` for the first file that failed."""
    lib = load_library()
    k = len(entries)
    p = np.ascontiguousarray(np.asarray(preds, dtype=np.float32).reshape(k, -1))
    if p.shape[1] != n * (n - 1) // 2 or len(out_paths) != k:
        raise ValueError(f"expected {k} x {n * (n - 1) // 2} distances and {k} paths")
    hs = (C.c_void_p * k)(*[e[0]._h for e in entries])
    fi = np.array([e[1] for e in entries], dtype=np.int32)
    paths = (C.c_char_p * k)(*[os.fsencode(q) for q in out_paths])
    trees = None
    if tree_paths is not None:
        if len(tree_paths) != k:
            raise ValueError(f"expected {k} tree paths")
        trees = (C.c_char_p * k)(*[os.fsencode(q) for q in tree_paths])
    status = np.zeros(k, dtype=np.int32)
    rc = lib.pf_phylip_write_batch(hs, fi.ctypes.data, k, n, p.ctypes.data, paths, trees, int(threads), status.ctypes.data)
    if rc != 0:
        raise ValueError(f"pf_phylip_write_batch: status {rc}")
    bad = np.flatnonzero(status)
    if bad.size:
        e = -int(status[bad[0]])
        raise OSError(e, os.strerror(e), out_paths[int(bad[0])] if tree_paths is None else f"{out_paths[int(bad[0])]} / {tree_paths[int(bad[0])]}")
