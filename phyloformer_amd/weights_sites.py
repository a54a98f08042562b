"""Site weights: pattern compression and bootstrap counts (host twins of ``csrc/pf_weights_host.h``).

Nothing in the network depends on a site's position and every reduction over sites is a plain sum, so an alignment in
which site ``l`` occurs ``w_l`` times is the alignment of its distinct sites with every sum over sites weighted by
``w_l`` and ``L`` replaced by ``W = sum_l w_l``.  The functions here build such tables; the
``native_*`` ones call the C twins (``pf_compress_sites``, ``pf_boot_counts``, ``pf_padded_sites``), which need no GPU.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .bootstrap import resample_sites


def padded_sites(K: int, L: int) -> int:
    """The one shape a launch over tables of up to ``K`` entries takes: ``min(L, 32 * ceil(K / 32))`` - a tile of the
    default kernels is 32 tokens, and coarse shapes keep the CLI's shape buckets few."""
    if K < 1 or K > L:
        raise ValueError(f"padded_sites needs 1 <= K <= L (got K={K}, L={L})")
    return min(L, 32 * ((K + 31) // 32))


def compress_sites(idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Distinct columns of ``uint8[N, L]`` in order of first occurrence: ``(first int32[K], count int32[K])`` -
    ``first[k]`` is the site where column ``k`` first stands, ``count[k]`` how often it occurs."""
    idx = np.ascontiguousarray(idx, dtype=np.uint8)
    if idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError(f"idx must be [N, L] with N, L >= 1, got shape {idx.shape}")
    seen = {}
    first, count = [], []
    cols = np.ascontiguousarray(idx.T)
    for l in range(cols.shape[0]):
        key = cols[l].tobytes()
        k = seen.get(key)
        if k is None:
            seen[key] = len(first)
            first.append(l)
            count.append(1)
        else:
            count[k] += 1
    return np.asarray(first, dtype=np.int32), np.asarray(count, dtype=np.int32)


def boot_counts(L: int, R: int, seed: int, r: int) -> Tuple[np.ndarray, np.ndarray]:
    """Replicate ``r`` (of ``R``) of ``bootstrap.resample_sites``' stream as ``(sites int32[K], counts int32[K])``: its
    distinct source sites, ascending, and how often it drew each."""
    if L < 1 or R < 1 or r < 0 or r >= R:
        raise ValueError(f"boot_counts needs L >= 1 and 0 <= r < R (got L={L}, R={R}, r={r})")
    sites, counts = np.unique(resample_sites(L, 1, seed, first=r)[0], return_counts=True)
    return sites.astype(np.int32), counts.astype(np.int32)


def pad_table(sites: np.ndarray, weights: np.ndarray, K: int) -> Tuple[np.ndarray, np.ndarray]:
    """One table row of ``K`` entries: the given sites and weights, then padding - site 0 with weight 0."""
    n = len(sites)
    if n > K:
        raise ValueError(f"{n} entries do not fit a row of {K}")
    s = np.zeros(K, dtype=np.int32)
    w = np.zeros(K, dtype=np.float32)
    s[:n] = sites
    w[:n] = weights
    return s, w


def compressed_table(idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(sites int32[Kp], weights float32[Kp])`` of one alignment: its distinct columns with their counts, padded to
    ``Kp = padded_sites(K, L)``.  ``forward_sites_weighted(idx, sites[None], weights[None])`` gives ``forward(idx)``'s
    distances to rounding."""
    first, count = compress_sites(idx)
    return pad_table(first, count, padded_sites(len(first), idx.shape[1]))


def boot_tables(L: int, R: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """The tables ``pf_bootstrap_weighted`` forwards: ``(sites int32[R, K], weights float32[R, K])``, every replicate's
    ``boot_counts`` padded to ``K = padded_sites(max_r distinct_r, L)``."""
    rows = [boot_counts(L, R, seed, r) for r in range(R)]
    K = padded_sites(max(len(s) for s, _ in rows), L)
    tabs = [pad_table(s, c, K) for s, c in rows]
    return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])


def expand(idx: np.ndarray, weights: np.ndarray) -> np.ndarray:
    """The alignment integer weights stand for: site ``l`` of ``uint8[N, L]`` repeated ``weights[l]`` times, in order."""
    w = np.asarray(weights)
    if np.any(w != np.round(w)) or np.any(w < 0):
        raise ValueError("expand needs non-negative integer weights")
    return np.repeat(np.asarray(idx), w.astype(np.int64), axis=-1)


# ---- the C twins (no GPU needed) ---------------------------------------------------------------------------------

def _fn(name: str):
    from .engine import load_library, symbol
    return symbol(load_library(), name)


def native_padded_sites(K: int, L: int) -> int:
    n = _fn("pf_padded_sites")(int(K), int(L))
    if n < 0:
        raise ValueError(f"padded_sites needs 1 <= K <= L (got K={K}, L={L})")
    return n


def native_compress_sites(idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    idx = np.ascontiguousarray(idx, dtype=np.uint8)
    if idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError(f"idx must be [N, L] with N, L >= 1, got shape {idx.shape}")
    N, L = idx.shape
    first = np.empty(L, dtype=np.int32)
    count = np.empty(L, dtype=np.int32)
    K = _fn("pf_compress_sites")(idx.ctypes.data, N, L, first.ctypes.data, count.ctypes.data)
    if K < 0:
        raise ValueError(f"pf_compress_sites failed with status {K}")
    return first[:K].copy(), count[:K].copy()


def native_boot_counts(L: int, R: int, seed: int, r: int) -> Tuple[np.ndarray, np.ndarray]:
    sites = np.empty(max(L, 1), dtype=np.int32)
    counts = np.empty(max(L, 1), dtype=np.int32)
    K = _fn("pf_boot_counts")(int(L), int(R), int(seed) & 0xFFFFFFFFFFFFFFFF, int(r), sites.ctypes.data, counts.ctypes.data)
    if K < 0:
        raise ValueError(f"boot_counts needs L >= 1 and 0 <= r < R (got L={L}, R={R}, r={r})")
    return sites[:K].copy(), counts[:K].copy()
