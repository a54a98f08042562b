"""A plain-Python model of what the default forward derives from an alignment's equal columns,
written from the definitions and without a call into the library:

  * ``classes``: what k_site_classes leaves - ``srep`` (every site's first equal column), ``ulist`` (the first
    occurrences, ascending) and ``ucount``;
  * ``split`` and ``compact_tiles``: the routing rule and the tile count of ``csrc/pf_layout.h``, the threshold's
    NUM / DEN read out of the header's text, so that the model cannot drift from the constants the kernels compile;
  * ``plan``: the record k_main_plan writes for a run of alignments (``main_plan_ints``).

And the alignment builders of the de-duplication tests: ``alignment`` draws its columns at random, ``alignment_simulated``
takes them from a simulated alignment - residues in the training distribution, for comparisons against the oracle.
"""
import os
import re

import numpy as np

LAYOUT_H = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                        "phyloformer_amd", "csrc", "pf_layout.h")
PLACEMENTS = ["front", "behind", "between"]


def classes(a):
    """uint8[N, L] -> (srep int32[L], ulist int32[K], K): first occurrences of equal columns."""
    seen, srep = {}, np.empty(a.shape[1], np.int32)
    for l in range(a.shape[1]):
        srep[l] = seen.setdefault(a[:, l].tobytes(), l)
    ulist = np.flatnonzero(srep == np.arange(a.shape[1])).astype(np.int32)
    assert len(ulist) == len(seen)
    return srep, ulist, len(seen)


_THRESHOLD = []


def threshold():
    """(NUM, DEN) of pf_layout.h: an alignment with K distinct columns of L splits iff K * DEN <= L * NUM."""
    if not _THRESHOLD:
        with open(LAYOUT_H) as fh:
            text = fh.read()
        num = re.findall(r"^#define\s+PF_MAIN_DEDUP_NUM\s+(\d+)", text, re.M)
        den = re.findall(r"^#define\s+PF_MAIN_DEDUP_DEN\s+(\d+)", text, re.M)
        assert len(num) == 1 and len(den) == 1, (num, den)
        _THRESHOLD.append((int(num[0]), int(den[0])))
    return _THRESHOLD[0]


def split(K, L, mode):
    """Does an alignment with K distinct columns of L take the split route under option main_dedup = mode?"""
    num, den = threshold()
    return mode == 2 or (mode == 1 and K * den <= L * num)


def compact_tiles(P, K):
    """Tiles of 32 over the P x K compacted tokens: consecutive tokens from K = 32 on, one ragged tile per row below."""
    return (P * K + 31) // 32 if K >= 32 else P


def plan(ucounts, P, L, mode):
    """(nf, ns, tiles, flist, slist, cpre) of a run: both lists ascending by alignment, cpre[i] the compact tiles in
    front of split alignment i, cpre[ns] their total."""
    flist = [b for b, K in enumerate(ucounts) if not split(int(K), L, mode)]
    slist = [b for b, K in enumerate(ucounts) if split(int(K), L, mode)]
    cpre = [0]
    for b in slist:
        cpre.append(cpre[-1] + compact_tiles(P, int(ucounts[b])))
    return len(flist), len(slist), cpre[-1], flist, slist, cpre


def read_plan(tap, B):
    """The "plan" debug tap (int32 view) of a run of B alignments in the form ``plan`` returns."""
    tap = np.asarray(tap)
    assert tap.dtype == np.int32 and tap.shape == (4 + 3 * B + 1,), (tap.dtype, tap.shape)
    nf, ns, tiles = (int(v) for v in tap[:3])
    assert 0 <= nf <= B and nf + ns == B, (nf, ns, B)
    flist, slist, cpre = tap[4:4 + nf], tap[4 + B:4 + B + ns], tap[4 + 2 * B:4 + 2 * B + ns + 1]
    return nf, ns, tiles, flist.tolist(), slist.tolist(), cpre.tolist()


# ---- alignments with a given number of distinct columns ----------------------------------------------------------------

def distinct_columns(rng, n, k):
    cols = {}
    while len(cols) < k:
        c = rng.integers(0, 22, n).astype(np.uint8)
        cols.setdefault(c.tobytes(), c)
    return np.stack(list(cols.values()), axis=1)          # [n, k]


def alignment(n, l, k, placement, seed=0, pool=None):
    """uint8[n, l] with exactly k distinct columns: random ones, or the first k of ``pool`` (uint8[n, >= k], distinct)."""
    rng = np.random.default_rng(100000 * n + 100 * l + k + seed)
    pool = distinct_columns(rng, n, k) if pool is None else pool[:, :k]
    rep = l - k
    if placement == "front":            # column 0, its repeats, then the other columns' first occurrences
        pick = np.concatenate([[0], np.zeros(rep, int), np.arange(1, k)])
    elif placement == "behind":         # every first occurrence, then repeats of any of them
        pick = np.concatenate([np.arange(k), rng.integers(0, k, rep)])
    else:                               # repeats scattered between the first occurrences, the last site a first one
        pick = np.full(l, -1)
        where = np.array([0]) if k == 1 else np.sort(np.concatenate([[0], rng.permutation(np.arange(1, l - 1))[:k - 2], [l - 1]]))
        pick[where.astype(int)] = np.arange(k)
        for s in np.flatnonzero(pick < 0):
            pick[s] = rng.integers(0, pick[:s].max() + 1)     # a column that stood in front already
    a = np.ascontiguousarray(pool[:, pick.astype(int)])
    assert a.shape == (n, l) and len({a[:, s].tobytes() for s in range(l)}) == k
    return a


_POOLS = {}


def simulated_pool(n):
    """The distinct columns of ``msa_sim.simulate_alignment(n, 1200, seed=2)`` in the order of their first occurrence."""
    if n not in _POOLS:
        from phyloformer_amd.msa_sim import simulate_alignment
        a = simulate_alignment(n, 1200, seed=2)
        pool = np.ascontiguousarray(a[:, classes(a)[1]])
        pool.setflags(write=False)
        _POOLS[n] = pool
    return _POOLS[n]


def alignment_simulated(n, l, k, placement, seed=0):
    """``alignment`` over columns of a simulated alignment of n sequences (760 distinct columns for n = 8)."""
    pool = simulated_pool(n)
    assert pool.shape[1] >= k, f"{pool.shape[1]} distinct simulated columns of {n} sequences, {k} wanted"
    return alignment(n, l, k, placement, seed, pool)
