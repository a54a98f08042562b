"""Felsenstein's bootstrap over alignment sites: the replicate stream and split supports on NJ trees.

Replicate ``r`` (0-based) of an alignment of ``L`` sites takes, at output position ``l``, the source site

    mix64(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31  (mod 2^64)
    key  = mix64(seed + 0x9E3779B97F4A7C15)          # the first SplitMix64 output for state `seed`
    z    = mix64(key ^ ((r << 32) | l))
    site = ((z >> 32) * L) >> 32                      # in [0, L)

The draw depends on ``(seed, r, l, L)`` only - not on the residues, the batch, the chunking or the device - so the
supports of a file depend on (weights, alignment, R, seed) alone.  ``resample_sites`` is the host twin of the device
kernel ``k_resample`` (csrc/pf_boot.hip.h), which ``pf_bootstrap`` runs chunk by chunk.

``support_newick_py`` is the Python twin of the native ``pf_nj_support_n`` (csrc/pf_hostio.cpp, bound as
``hostio.nj_support``): the NJ tree of the alignment's own distances with, after the ``)`` of every internal node, the
integer percent ``(200 c + R) // (2 R)`` of the R replicate trees that contain the node's split.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from .nj import join_splits, neighbor_joining, newick_of_joins, nj_joins
from .phylip import vec_to_matrix

GOLDEN_GAMMA = 0x9E3779B97F4A7C15
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix64(z: np.ndarray) -> np.ndarray:
    """SplitMix64's finaliser on ``uint64`` arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * _M1
        z = z ^ (z >> np.uint64(27))
        z = z * _M2
        z = z ^ (z >> np.uint64(31))
    return z


def stream_key(seed: int) -> int:
    return int(mix64(np.uint64((int(seed) + GOLDEN_GAMMA) & 0xFFFFFFFFFFFFFFFF)))


def resample_sites(L: int, R: int, seed: int, first: int = 0) -> np.ndarray:
    """``int64[R][L]``: the source sites of replicates ``first .. first + R - 1``."""
    L, R, first = int(L), int(R), int(first)
    if L < 1 or R < 0 or first < 0 or L >= 1 << 32 or first + R > 1 << 32:
        raise ValueError(f"bad stream arguments L={L} R={R} first={first}")
    key = np.uint64(stream_key(seed))
    r = np.arange(first, first + R, dtype=np.uint64)[:, None]
    l = np.arange(L, dtype=np.uint64)[None, :]
    z = mix64(key ^ ((r << np.uint64(32)) | l))
    return (((z >> np.uint64(32)) * np.uint64(L)) >> np.uint64(32)).astype(np.int64)


def resample(idx: np.ndarray, R: int, seed: int) -> np.ndarray:
    """``uint8[B][N][L]`` (or ``[N][L]``) -> the replicates ``uint8[B][R][N][L]`` (or ``[R][N][L]``)."""
    idx = np.asarray(idx, dtype=np.uint8)
    sites = resample_sites(idx.shape[-1], R, seed)
    out = idx[..., sites]                       # [..., N, R, L]
    return np.ascontiguousarray(np.moveaxis(out, -2, -3))


def support_percent(count: int, R: int) -> int:
    return (200 * int(count) + int(R)) // (2 * int(R))


def support_newick_py(preds: np.ndarray, reps: np.ndarray, ids: Sequence[str], clamp_negative: bool = True) -> str:
    """NJ tree of ``preds [P]`` (the ``.nj.nwk`` text) with a support label on every internal node, counted over the
    NJ trees of ``reps [R][P]``.  Splits are bitsets over sequence indices, so duplicate ids are no problem."""
    n = len(ids)
    preds = np.asarray(preds, dtype=np.float32).reshape(-1)
    reps = np.asarray(reps, dtype=np.float32)
    if reps.ndim != 2 or reps.shape[0] < 1 or reps.shape[1] != preds.size:
        raise ValueError(f"expected replicates [R >= 1][{preds.size}], got {reps.shape}")
    dm = vec_to_matrix(preds, n).astype(np.float64)
    if n <= 3:
        return neighbor_joining(dm, ids, clamp_negative)      # no internal split to support
    R = reps.shape[0]
    joins, final = nj_joins(dm)
    splits = join_splits(joins, n)
    counts = [0] * len(splits)
    for rep in reps:
        seen = set(join_splits(nj_joins(vec_to_matrix(rep, n).astype(np.float64))[0], n))
        for t, s in enumerate(splits):
            counts[t] += s in seen
    labels: List[int] = [support_percent(c, R) for c in counts]
    return newick_of_joins(ids, joins, final, clamp_negative, labels)
