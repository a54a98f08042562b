"""Delta scores for the ``--delta`` flag of the CLI: how tree-like a vector of distances is (the delta plot of Holland,
Huber, Dress & Moulton 2002; ``delta.plot`` of R's ape).

The distances of a tree satisfy the four-point condition: of the three sums ``d_ab + d_cd``, ``d_ac + d_bd``,
``d_ad + d_bc`` of a quartet the two largest are equal.  With ``m1 >= m2 >= m3`` the sums in order, ``delta = (m1 - m2) /
(m1 - m3)`` is 0 for such a quartet and 1 at the most; it is 0 by definition where ``m1 == m3``.

``delta_py`` is the statement the native twins are held to (``csrc/pf_delta_host.h``, ``csrc/pf_delta.hip.h``, DESIGN.md
section 30): the sums are single float64 additions of float32 distances, the order is found by comparisons, the quotient
is one float64 division, and ``q = rint(delta 2^30)`` - ties to even - is an integer in ``[0, 2^30]``.  Everything after
``q`` is integer arithmetic, so the arrays do not depend on the order of the quartets: the host visits each once, the
device six times, and the three agree bit for bit.
"""
from __future__ import annotations

from itertools import combinations
from math import comb
from typing import NamedTuple, Sequence, Tuple

import numpy as np

Q_SHIFT = 30
Q_ONE = 1 << Q_SHIFT
MIN_SEQS, MAX_SEQS = 4, 2048      # 3 C(N-1, 3) 2^30 must stay below 2^63
MAX_BINS = 64
BINS = 20                         # the CLI's histogram: ape's default


def n_of_pairs(pairs: int) -> int:
    """The number of sequences with ``pairs`` pairs; 0 if there is none."""
    n = (1 + int(round((1 + 8 * pairs) ** 0.5))) // 2
    return n if n * (n - 1) // 2 == pairs else 0


def refuse(b: int, n: int, bins: int):
    """What the three entry points refuse, with their messages."""
    if not MIN_SEQS <= n <= MAX_SEQS:
        raise ValueError(f"delta scores take {MIN_SEQS} <= N <= {MAX_SEQS} sequences (got {n})")
    if b < 1:
        raise ValueError(f"bad dimensions B={b} N={n}")
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"delta scores take 1 <= K <= {MAX_BINS} bins (got {bins})")


def delta_arrays(preds, bins: int, n: int = 0):
    """The arguments of the three ``pf_delta`` entry points, checked: ``(preds float32[B, P_n], (B, n), single, zeroed
    (pair_sum, hist, nonfinite))``; ``n`` = 0 takes the number of sequences from the width."""
    p = np.ascontiguousarray(np.asarray(preds, dtype=np.float32))
    single = p.ndim == 1
    if single:
        p = p[None, :]
    if p.ndim != 2:
        raise ValueError(f"expected distances [B, P] or [P], got {p.shape}")
    n = int(n) or n_of_pairs(p.shape[1])
    if n * (n - 1) // 2 != p.shape[1]:
        raise ValueError(f"expected {n * (n - 1) // 2} distances for {n} sequences, got {p.shape[1]}")
    b, bins = p.shape[0], int(bins)
    refuse(b, n, bins)
    return p, (b, n), single, (np.zeros((b, p.shape[1]), dtype=np.int64), np.zeros((b, bins), dtype=np.int64),
                               np.zeros(b, dtype=np.uint8))


def quartet_q(s1: np.float64, s2: np.float64, s3: np.float64) -> int:
    """``q`` of a quartet's three sums (finite float64 scalars)."""
    hi, lo = (s2, s1) if s1 < s2 else (s1, s2)
    m1 = s3 if hi < s3 else hi
    m3 = s3 if s3 < lo else lo
    t = s3 if s3 < hi else hi
    m2 = t if lo < t else lo
    den = m1 - m3
    if den == 0.0:
        return 0
    return int(np.rint((m1 - m2) / den * np.float64(Q_ONE)))


def delta_py(pred: np.ndarray, n: int, bins: int = BINS) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The statement: ``pred float32 [P_n]`` (pairs ``i < j`` in lexicographic order) → ``(pair_sum int64 [P_n], hist int64
    [bins], nonfinite uint8 scalar)``.  ``pair_sum[i, j]`` is the sum of ``q`` over the quartets that hold ``i`` and ``j``,
    ``hist`` the quartets per bin ``min(bins - 1, (q bins) >> 30)``.  A NaN or an infinity in ``pred``: the flag and zeros."""
    pred = np.asarray(pred, dtype=np.float32)
    refuse(1, n, bins)
    if pred.shape != (n * (n - 1) // 2,):
        raise ValueError(f"expected {n * (n - 1) // 2} distances for {n} sequences, got {pred.shape}")
    pair_sum = np.zeros(pred.size, dtype=np.int64)
    hist = np.zeros(bins, dtype=np.int64)
    if not np.isfinite(pred).all():
        return pair_sum, hist, np.uint8(1)
    d = pred.astype(np.float64)
    index = {pair: k for k, pair in enumerate(combinations(range(n), 2))}
    for a, b, c, e in combinations(range(n), 4):
        ab, cd, ac, be, ae, bc = index[a, b], index[c, e], index[a, c], index[b, e], index[a, e], index[b, c]
        q = quartet_q(d[ab] + d[cd], d[ac] + d[be], d[ae] + d[bc])
        for k in (ab, cd, ac, be, ae, bc):
            pair_sum[k] += q
        hist[min(bins - 1, (q * bins) >> Q_SHIFT)] += 1
    return pair_sum, hist, np.uint8(0)


class Scores(NamedTuple):
    """The means of delta of one source: over the quartets that hold a sequence, over those that hold a pair, over all;
    ``quartets`` = C(n, 4).  ``nan`` where there is no quartet."""
    taxon: np.ndarray       # float64 [n]
    pair: np.ndarray        # float64 [P_n]
    overall: float
    quartets: int


def delta_scores(pair_sum: np.ndarray, hist: np.ndarray, n: int) -> Scores:
    """The derived means of one source's ``pair_sum [P_n]`` (``hist`` is checked against the number of quartets): the sums
    over a sequence's pairs and over all pairs hold every quartet 3 and 6 times, and the quotients are Python's ``int /
    int``."""
    pair_sum = np.asarray(pair_sum, dtype=np.int64)
    quartets = comb(n, 4)
    if int(np.asarray(hist).sum()) != quartets:
        raise ValueError(f"the histogram counts {int(np.asarray(hist).sum())} quartets, {n} sequences have {quartets}")
    i, j = np.triu_indices(n, k=1)
    taxon_sum = [0] * n
    for a, b, s in zip(i.tolist(), j.tolist(), pair_sum.tolist()):
        taxon_sum[a] += s
        taxon_sum[b] += s
    total = sum(pair_sum.tolist())
    if any(s % 3 for s in taxon_sum) or total % 6:
        raise ValueError("pair sums that are not those of whole quartets")
    per_taxon, per_pair = comb(n - 1, 3) * Q_ONE, comb(n - 2, 2) * Q_ONE
    return Scores(np.array([s // 3 / per_taxon for s in taxon_sum], dtype=np.float64),
                  np.array([s / per_pair for s in pair_sum.tolist()], dtype=np.float64),
                  total // 6 / (quartets * Q_ONE), quartets)


def no_scores(n: int) -> Scores:
    """The scores of a file without a quartet (fewer than 4 sequences) or with distances that are not finite."""
    return Scores(np.full(n, np.nan), np.full(n * (n - 1) // 2, np.nan), float("nan"), comb(n, 4))


# ---- the three files of --delta -------------------------------------------------------------------------------------

def delta_tsv(ids: Sequence[str], scores: Scores) -> str:
    """``<stem>.delta.tsv``: a comment line with the overall mean and the number of quartets, then one line per sequence -
    ``index``, ``id``, ``delta`` (the mean over the quartets that hold it), ``relative`` (delta / its mean over the
    sequences; ``nan`` where that mean is 0 or there is none)."""
    mean = float(np.mean(scores.taxon)) if len(scores.taxon) else float("nan")
    lines = [f"# overall_delta={scores.overall:.10f}\tquartets={scores.quartets}\n", "index\tid\tdelta\trelative\n"]
    for k, (name, x) in enumerate(zip(ids, scores.taxon.tolist())):
        rel = x / mean if mean > 0 else float("nan")
        lines.append(f"{k}\t{name}\t{x:.10f}\t{rel:.10f}\n")
    return "".join(lines)


def hist_tsv(hist: np.ndarray) -> str:
    """``<stem>.delta.hist.tsv``: ``bin``, ``from``, ``to``, ``quartets``, ``share`` (``nan`` without a quartet)."""
    hist = np.asarray(hist, dtype=np.int64)
    k, total = len(hist), int(hist.sum())
    lines = ["bin\tfrom\tto\tquartets\tshare\n"]
    for b, c in enumerate(hist.tolist()):
        share = c / total if total else float("nan")
        lines.append(f"{b}\t{b / k:.4f}\t{(b + 1) / k:.4f}\t{c}\t{share:.10f}\n")
    return "".join(lines)


def pair_vector(scores: Scores) -> np.ndarray:
    """``<stem>.delta.phy``'s values: the per-pair means as the float32 vector a PHYLIP writer takes."""
    return scores.pair.astype(np.float32)


def parse_delta_tsv(text: str):
    """``(overall, quartets, ids, delta, relative)`` of a ``<stem>.delta.tsv``."""
    head, _names, *rows = text.splitlines()
    fields = dict(f.split("=") for f in head[2:].split("\t"))
    cols = [r.split("\t") for r in rows]
    return (float(fields["overall_delta"]), int(fields["quartets"]), [c[1] for c in cols],
            np.array([float(c[2]) for c in cols]), np.array([float(c[3]) for c in cols]))


def parse_hist_tsv(text: str) -> np.ndarray:
    """The counts of a ``<stem>.delta.hist.tsv``."""
    return np.array([int(r.split("\t")[3]) for r in text.splitlines()[1:]], dtype=np.int64)
