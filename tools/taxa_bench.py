#!/usr/bin/env python3
"""Leave-one-out rates.  Per shape (20 x 200 B = 8, 60 x 500 B = 1):

  loo_sets_per_s         pf_forward_leave_one_out: cuts/s (host buffers in and out; the whole alignments' forward, the
                         cuts made on the device, re-check, statistics reduced on the device)
  cut_fwd_sets_per_s     the way without the entry point: pf_forward on the B alignments, then pf_forward on the host-cut
                         [B * N][N - 1][L] batch, upload of every cut included (the cut itself and the statistics, numpy
                         on the host, are timed apart: host_cut_ms, host_stats_ms)
  loo_over_cut_fwd       time of pf_forward_leave_one_out / time of the two pf_forward calls (< 1: faster)
  upload_bytes           source bytes the entry point uploads / bytes the other way uploads
  gather_taxa_ms, gather_taxa_share, loo_stats_ms, loo_stats_share
                         k_gather_taxa's and the reduction's time and share of the GPU time of one call (option
                         "profile" = 1: HIP events)

Best of --repeat.  One JSON line per shape.  GPU only.

    python tools/taxa_bench.py [--repeat 3] [--shapes 20x200x8,60x500x1]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--shapes", default="20x200x8,60x500x1", help="NxLxB,... (B source alignments per call)")
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.taxa import cut_taxa, leave_one_out_sets, loo_stats
    from phyloformer_amd.weights import load_weights

    names = ["embed", "rowfin", "colstats", "colfin", "main", "allreduce", "precise", "generic", "resample", "gather",
             "site_moments", "gather_taxa", "loo_stats"]
    w = load_weights(os.path.join(REPO, "models", "pf.ckpt"))
    with Engine(w, 0) as e:
        for spec in args.shapes.split(","):
            N, L, B = (int(v) for v in spec.split("x"))
            idx = simulate_batch(B, N, L, seed=1)
            sets = leave_one_out_sets(N)
            rep = {"shape": f"{N}x{L}", "B": B, "sets": B * N}
            t_loo = timed(lambda: e.forward_leave_one_out(idx), args.repeat)
            rep["loo_sets_per_s"] = round(B * N / t_loo, 1)
            rep["host_cut_ms"] = round(1e3 * timed(lambda: cut_taxa(idx, sets), args.repeat), 3)
            cut = cut_taxa(idx, sets).reshape(B * N, N - 1, L)

            def by_hand():
                return e.forward(idx), e.forward(cut)
            t_cut = timed(by_hand, args.repeat)
            rep["cut_fwd_sets_per_s"] = round(B * N / t_cut, 1)
            rep["loo_over_cut_fwd"] = round(t_loo / t_cut, 4)
            rep["upload_bytes"] = [2 * int(idx.nbytes), int(idx.nbytes) + int(cut.nbytes)]
            out, infl, shift, ctx, loo = e.forward_leave_one_out(idx, keep_loo=True)
            full, cuts = by_hand()
            rep["bit_identical"] = bool(np.array_equal(out.view(np.uint32), full.view(np.uint32)) and
                                        np.array_equal(loo.reshape(B * N, -1).view(np.uint32), cuts.view(np.uint32)))
            rep["host_stats_ms"] = round(1e3 * timed(lambda: loo_stats(out, loo), args.repeat), 3)
            want = loo_stats(out, loo)
            rep["stats_max_abs_diff"] = float(max(np.abs(a.astype(np.float64) - b).max() for a, b in zip((infl, shift, ctx), want)))
            e.set_option("profile", 1)
            e.profile_reset()
            e.forward_leave_one_out(idx)
            ms = {k: e.profile_get(k)[1] for k in names}
            e.set_option("profile", 0)
            total = max(1e-9, sum(ms.values()))
            for k in ("gather_taxa", "loo_stats"):
                rep[f"{k}_ms"] = round(ms[k], 4)
                rep[f"{k}_share"] = round(ms[k] / total, 5)
            print(json.dumps(rep), flush=True)


if __name__ == "__main__":
    main()
