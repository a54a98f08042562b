#!/usr/bin/env python3
"""Generate ``tests/golden/loo.npz``: the reference's own distances for two shipped MSAs and each of their
leave-one-out cuts.

Runs the REFERENCE on the CPU the way ``oracle/gen_golden.py`` does (build container only: the reference is not part
of this repository), checkpoint ``pf``.  Only data is written: per case the residue indices ``uint8 [N][L]``, the
reference's distances of the whole alignment ``full float32 [P]`` and of the alignment without row ``t``, remaining rows
in order, ``loo float32 [N][P1]``, and ``influence``, ``shift``, ``context`` computed from those in float64 HERE, by
explicit loops over (t, i, j) - independent of phyloformer_amd/taxa.py - and stored as float64.

    0_20_tips        the whole alignment and its 20 cuts
    1_30_tips_12     the first 12 rows of 1_30_tips and their 12 cuts

    python tools/gen_golden_loo.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CASES = (("0_20_tips", "0_20_tips", None), ("1_30_tips_12", "1_30_tips", 12))


def stats(full, loo):
    """The definitions, pair by pair: pairs of N rows and of the N - 1 rows of a cut are numbered by walking the
    row-major upper triangle."""
    N = loo.shape[0]
    number = {}
    for i in range(N):
        for j in range(i + 1, N):
            number[(i, j)] = len(number)
    infl, shift, ssq = np.zeros(N), np.zeros(N), np.zeros(len(number))
    for t in range(N):
        rows = [r for r in range(N) if r != t]
        q, deltas = 0, []
        for a in range(N - 1):
            for b in range(a + 1, N - 1):
                p = number[(rows[a], rows[b])]
                d = float(loo[t][q]) - float(full[p])
                deltas.append(d)
                ssq[p] += d * d
                q += 1
        deltas = np.asarray(deltas)
        infl[t], shift[t] = np.sqrt((deltas ** 2).mean()), deltas.mean()
    return infl, shift, np.sqrt(ssq / (N - 2))


def main():
    from oracle.gen_golden import GOLD, _import_reference, _load_model, _onehot
    from phyloformer_amd.fasta import load_alignment
    torch, Phyloformer, _ref_load, _stub = _import_reference()
    model = _load_model(torch, Phyloformer, "pf")

    def dist(a):
        with torch.no_grad():
            return model(_onehot(torch, a)).numpy().astype(np.float32).reshape(-1)

    out = {}
    for key, stem, rows in CASES:
        idx, _ids = load_alignment(os.path.join(REPO, "data", "testdata", "msas", f"{stem}.fa"))
        idx = np.ascontiguousarray(idx[:rows] if rows else idx)
        N = idx.shape[0]
        full = dist(idx)
        loo = np.stack([dist(np.ascontiguousarray(np.delete(idx, t, axis=0))) for t in range(N)])
        infl, shift, ctx = stats(full, loo)
        out[f"{key}/idx"], out[f"{key}/full"], out[f"{key}/loo"] = idx, full, loo
        out[f"{key}/influence"], out[f"{key}/shift"], out[f"{key}/context"] = infl, shift, ctx
        print(key, idx.shape, full.shape, loo.shape, "influence", infl.min(), infl.max())
    path = os.path.join(GOLD, "loo.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
