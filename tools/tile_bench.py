#!/usr/bin/env python3
"""Tiled inference against the separate calls it replaces, and what tiling does to the answer.

Time, per shape N x L with context M, best of --repeat (one JSON line per shape):

  tiled_ms        one pf_forward_tiled call (one upload, sets cut and combined on the device)
  separate_ms     the same sets forwarded by pf_forward_taxa, one call per set size, and tile.combine on the host
  combine_ms      k_tile_combine's HIP-event time in a profiled call of its own, and its share of tiled_ms
  untiled_ms      pf_forward of the whole alignment where the cap admits it (N <= 200), tiled_over_untiled next to the
                  token ratio of the sets it should track

The results of both are compared bit for bit before anything is timed.  N beyond the cap: the separate path needs
"max_seqs" = 0 (pf_forward_taxa checks N), so the whole shape runs with the cap lifted.

The answer (--answer, one JSON line per file): the five shipped 50-tip alignments with M = 26 - mean and maximum absolute
difference between tiled and untiled distances for within-group and cross-group pairs, and the normalised Robinson-
Foulds distance of both NJ trees to the true tree.  Descriptive: these numbers gate nothing.

Reads nothing outside the repository.  GPU only.

    python tools/tile_bench.py [--shapes 200x500x50,1000x300x100] [--repeat 3] [--answer]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, repeat):
    fn()                                   # warm-up (workspaces, code objects)
    best = float("inf")
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def separate(e, idx, M):
    """The sets through pf_forward_taxa, one call per set size, combined on the host."""
    from phyloformer_amd import tile as TL
    p = TL.plan(idx.shape[-2], M)
    rows = [p.set_rows(k) for k in range(p.S)]
    sets = [None] * p.S
    for m in sorted({len(r) for r in rows}):
        ks = [k for k in range(p.S) if len(rows[k]) == m]
        res = e.forward_taxa(idx, np.stack([rows[k] for k in ks]).astype(np.int32))
        for j, k in enumerate(ks):
            sets[k] = res[..., j, :]
    return TL.combine(sets, p.N, M)


def bench_shapes(e, shapes, repeat):
    from phyloformer_amd import tile as TL
    from phyloformer_amd.msa_sim import simulate_batch
    for spec in shapes.split(","):
        N, L, M = (int(v) for v in spec.split("x"))
        idx = simulate_batch(1, N, L, seed=1)
        e.set_option("max_seqs", 0 if N > 200 else 200)
        p = TL.plan(N, M)
        got, want = e.forward_tiled(idx, M), separate(e, idx, M)
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        t_tiled = timed(lambda: e.forward_tiled(idx, M), repeat)
        t_sep = timed(lambda: separate(e, idx, M), repeat)
        e.set_option("profile", 1)
        e.profile_reset()
        e.forward_tiled(idx, M)
        launches, combine_ms = e.profile_get("tile_combine")
        e.set_option("profile", 0)
        tokens = sum(len(p.set_rows(k)) * (len(p.set_rows(k)) - 1) // 2 for k in range(p.S)) / (N * (N - 1) // 2)
        line = {"shape": f"{N}x{L}", "M": M, "G": p.G, "sets": p.S, "tiled_ms": round(1e3 * t_tiled, 3),
                "separate_ms": round(1e3 * t_sep, 3), "tiled_over_separate": round(t_tiled / t_sep, 4),
                "combine_launches": launches, "combine_ms": round(combine_ms, 4),
                "combine_share": round(combine_ms / (1e3 * t_tiled), 6), "token_ratio": round(tokens, 4),
                "two_g_minus_1_over_g": round(2 * (p.G - 1) / p.G, 4), "rechecked": e.rechecked_count()}
        if N <= 200:
            t_whole = timed(lambda: e.forward(idx), repeat)
            line.update(untiled_ms=round(1e3 * t_whole, 3), tiled_over_untiled=round(t_tiled / t_whole, 4))
        print(json.dumps(line), flush=True)
    e.set_option("max_seqs", 200)


def answer(e, M=26):
    from phyloformer_amd import tile as TL
    from phyloformer_amd import treecmp as TC
    from phyloformer_amd.fasta import load_alignment
    from phyloformer_amd.nj import neighbor_joining
    from phyloformer_amd.phylip import vec_to_phylip
    for k in range(5):
        stem = f"{k}_50_tips"
        idx, ids = load_alignment(os.path.join(REPO, "data", "testdata", "msas", f"{stem}.fa"))
        with open(os.path.join(REPO, "data", "testdata", "trees", f"{stem}.nwk")) as fh:
            truth = TC.parse_newick(fh.read())
        whole = e.forward(idx)
        tiled, spread = e.forward_tiled(idx, M)
        grp = TL.plan(len(ids), M).groups_of_rows()
        iu, ju = np.triu_indices(len(ids), k=1)
        same = grp[iu] == grp[ju]
        diff = np.abs(tiled.astype(np.float64) - whole)

        def nrf(vec):
            tree = neighbor_joining(vec_to_phylip(vec, ids)[0].astype("float64"), ids)
            return round(TC.robinson_foulds(TC.parse_newick(tree), truth)[1], 4)

        print(json.dumps({"file": stem, "M": M, "mean_distance": round(float(whole.mean()), 6),
                          "within_mean_abs": round(float(diff[same].mean()), 6), "within_max_abs": round(float(diff[same].max()), 6),
                          "cross_mean_abs": round(float(diff[~same].mean()), 6), "cross_max_abs": round(float(diff[~same].max()), 6),
                          "within_mean_spread": round(float(spread[same].mean()), 6),
                          "nrf_untiled": nrf(whole), "nrf_tiled": nrf(tiled)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--shapes", default="200x500x50,1000x300x100", help="NxLxM,... (one alignment per call)")
    ap.add_argument("--answer", action="store_true", help="also the tiled-against-untiled study on the shipped 50-tip files")
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.weights import load_weights

    w = load_weights(os.path.join(REPO, "models", "pf.ckpt"))
    with Engine(w, 0) as e:
        if args.shapes:
            bench_shapes(e, args.shapes, args.repeat)
        if args.answer:
            answer(e)


if __name__ == "__main__":
    main()
