"""Site-window scans on the host: the window rule, the host twin of the device gather, and the per-window summary.

``window_starts`` mirrors ``pf_window_count`` / ``pf_window_start`` (include/phyloformer_amd.h), ``cut_sites`` mirrors
``k_gather_sites`` (csrc/pf_sites.hip.h): ``Engine.forward_windows`` / ``Engine.forward_sites`` promise the bits of
``Engine.forward(cut_sites(idx, sites))``.  The summary table (``<stem>.windows.tsv`` of ``infer_alns.py --windows``)
compares every window's neighbour-joining tree with the previous window's and with the whole alignment's.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np


def window_starts(L: int, W: int, step: Optional[int] = None) -> List[int]:
    """First sites (0-based) of the windows of ``W`` sites over ``L``: ``0, step, 2 * step, ...`` while
    ``start + W <= L``; if the last of them ends before ``L``, one more window anchored at ``L - W``, so that every
    site is covered.  ``W == L`` gives one window; ``step`` defaults to ``W`` (non-overlapping)."""
    L, W = int(L), int(W)
    step = W if step is None else int(step)
    if W < 1:
        raise ValueError(f"window width must be >= 1 (got {W})")
    if step < 1:
        raise ValueError(f"window step must be >= 1 (got {step})")
    if W > L:
        raise ValueError(f"window width {W} exceeds the alignment's {L} sites")
    starts = list(range(0, L - W + 1, step))
    if starts[-1] + W < L:
        starts.append(L - W)
    return starts


def window_sites(L: int, W: int, step: Optional[int] = None) -> np.ndarray:
    """The windows as a site table ``int32[S, W]`` (what ``forward_sites`` takes)."""
    st = np.asarray(window_starts(L, W, step), dtype=np.int32)
    return st[:, None] + np.arange(int(W), dtype=np.int32)[None, :]


def cut_sites(idx: np.ndarray, sites: np.ndarray) -> np.ndarray:
    """``uint8[B, N, L]``, ``int[S, K]`` → ``uint8[B, S, N, K]`` (``[N, L]`` → ``[S, N, K]``): derived alignment ``s``
    of source ``b`` is ``idx[b][:, sites[s]]``.  Entries outside ``[0, L)`` raise ``ValueError`` (never wrapped)."""
    idx = np.asarray(idx, dtype=np.uint8)
    tab = np.asarray(sites)
    if tab.ndim != 2 or tab.dtype.kind not in "iu":
        raise ValueError(f"sites must be an integer array [S, K], got {tab.dtype} {tab.shape}")
    L = idx.shape[-1]
    if tab.size and (tab.min() < 0 or tab.max() >= L):
        raise ValueError(f"site outside [0, {L})")
    return np.ascontiguousarray(np.moveaxis(idx[..., tab], -2, -3))


def window_label(L: int, start: int, W: int) -> str:
    """``w<first>-<last>``: 1-based inclusive site numbers, zero-padded to the width of ``L``."""
    d = len(str(int(L)))
    return f"w{start + 1:0{d}d}-{start + W:0{d}d}"


TSV_HEADER = "first\tlast\tmean_distance\trf_prev\trf_full\n"


def _rf(a, b) -> str:
    from .treecmp import robinson_foulds
    if a is None or b is None:
        return "NA"
    try:
        return str(robinson_foulds(a, b)[0])
    except ValueError:          # duplicate sequence ids: splits are not defined on names
        return "NA"


def _tree(newick: str):
    from .treecmp import parse_newick
    try:
        return parse_newick(newick)
    except ValueError:          # an id the Newick grammar cannot carry unquoted
        return None


def summary_tsv(starts: Sequence[int], W: int, window_preds: np.ndarray, window_trees: Sequence[str], full_tree: str) -> str:
    """The text of ``<stem>.windows.tsv``: one row per window - ``first last`` (1-based, inclusive), the mean of the
    window's predicted distances (float64 mean of the float32 values, ``%.10f``), and the Robinson-Foulds distances
    (``treecmp.robinson_foulds``) of the window's NJ tree to the previous window's (``NA`` for the first) and to the
    whole alignment's.  A tree ``treecmp`` cannot compare (duplicate or unparsable ids) gives ``NA``."""
    full = _tree(full_tree)
    rows, prev = [TSV_HEADER], None
    for k, st in enumerate(starts):
        t = _tree(window_trees[k])
        mean = float(np.asarray(window_preds[k], dtype=np.float64).mean()) if np.size(window_preds[k]) else 0.0
        rows.append(f"{st + 1}\t{st + W}\t{mean:.10f}\t{_rf(t, prev) if k else 'NA'}\t{_rf(t, full)}\n")
        prev = t
    return "".join(rows)


def parse_windows_arg(text: str) -> Tuple[int, int]:
    """``W[:STEP]`` of ``--windows`` → ``(W, step)``; ``STEP`` defaults to ``W``."""
    parts = str(text).split(":")
    if len(parts) not in (1, 2):
        raise ValueError(f"expected W[:STEP], got {text!r}")
    W = int(parts[0])
    step = int(parts[1]) if len(parts) == 2 else W
    if W < 1 or step < 1:
        raise ValueError(f"window width and step must be >= 1 (got {text!r})")
    return W, step
