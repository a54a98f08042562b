#!/usr/bin/env python3
"""Site bootstrap rates.  Per shape (20 x 200, 60 x 500, and 200 x 500 for the host side), R = 100:

  boot_reps_per_s        pf_bootstrap replicates/s (host buffers in and out, resampling on the device, re-check)
  fwd_dev_alns_per_s     pf_forward_device alignments/s on the same B x R replicates, prebuilt in HBM
  boot_over_fwd          time of pf_bootstrap / time of pf_forward_device on the same replicates
  rechecked_per_call     replicates the range re-check recomputed in float64 (option "recheck_above"), and
  boot_over_fwd_no_recheck   the ratio with the re-check off
  resample_share         k_resample's share of the GPU time of a pf_bootstrap call (option "profile" = 1)
  boot_ms_per_aln        pf_bootstrap time per source alignment (R replicates)
  lone_ms_per_aln        the same R replicates as R lone pf_forward calls of one alignment each
  support_ms_1t / _wt    host supports per alignment (pf_nj_support_n: R + 1 NJ trees), 1 thread / writer threads

One JSON line per shape.  GPU only.

    python tools/bootstrap_bench.py [--reps 100] [--repeat 3] [--writer-threads 4]
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
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--writer-threads", type=int, default=4)
    ap.add_argument("--shapes", default="20x200x8,60x500x2,200x500x1", help="NxLxB,... (B source alignments per call)")
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.hostio import nj_support
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.weights import load_weights

    names = ["embed", "rowfin", "colstats", "colfin", "main", "allreduce", "precise", "generic", "resample"]
    R = args.reps
    w = load_weights(os.path.join(REPO, "models", "pf.ckpt"))
    with Engine(w, 0) as e:
        for spec in args.shapes.split(","):
            N, L, B = (int(v) for v in spec.split("x"))
            P = N * (N - 1) // 2
            idx = simulate_batch(B, N, L, seed=1)
            seed = 5
            rep = {"shape": f"{N}x{L}", "B": B, "R": R}
            t_boot = timed(lambda: e.bootstrap(idx, R, seed), args.repeat)
            rep["boot_reps_per_s"] = round(B * R / t_boot, 1)
            rep["boot_ms_per_aln"] = round(1e3 * t_boot / B, 3)
            # the same replicates prebuilt on the device, then pf_forward_device alone
            d_src, d_rep, d_out = e.malloc(idx.nbytes), e.malloc(B * R * N * L), e.malloc(B * R * P * 4)
            try:
                e.h2d(d_src, idx)
                e.resample_sites_device(d_src, B, N, L, 0, R, seed, d_rep)
                e.synchronize()

                def fwd():
                    e.forward_device(d_rep, B * R, N, L, d_out)
                    e.synchronize()
                t_fwd = timed(fwd, args.repeat)
            finally:
                for p in (d_src, d_rep, d_out):
                    e.free(p)
            rep["fwd_dev_alns_per_s"] = round(B * R / t_fwd, 1)
            rep["boot_over_fwd"] = round(t_boot / t_fwd, 4)
            # replicates the range re-check recomputed in float64 per call, and the ratio without the re-check
            e.profile_reset()
            e.bootstrap(idx, R, seed)
            rep["rechecked_per_call"] = e.rechecked_count()
            e.set_option("recheck_above", 0)
            rep["boot_over_fwd_no_recheck"] = round(timed(lambda: e.bootstrap(idx, R, seed), args.repeat) / t_fwd, 4)
            e.set_option("recheck_above", 8)
            # k_resample's share of the GPU time
            e.set_option("profile", 1)
            e.profile_reset()
            e.bootstrap(idx, R, seed)
            ms = {k: e.profile_get(k)[1] for k in names}
            e.set_option("profile", 0)
            rep["resample_ms"] = round(ms["resample"], 4)
            rep["resample_share"] = round(ms["resample"] / max(1e-9, sum(ms.values())), 5)
            # R lone forwards of one alignment each
            reps = e.bootstrap(idx[:1], R, seed)[0]
            from phyloformer_amd.bootstrap import resample
            host_reps = resample(idx[0], R, seed)
            if N * L <= 20 * 200 * 4:
                t_lone = timed(lambda: [e.forward(host_reps[r][None]) for r in range(R)], 1)
                rep["lone_ms_per_aln"] = round(1e3 * t_lone, 3)
            # host supports of one alignment (R + 1 NJ trees)
            pred = e.forward(idx[:1])[0]
            ids = [f"t{i}" for i in range(N)]
            rep["support_ms_1t"] = round(1e3 * timed(lambda: nj_support(pred, reps, ids, threads=1), 1), 3)
            rep["support_ms_wt"] = round(1e3 * timed(lambda: nj_support(pred, reps, ids, threads=args.writer_threads), 1), 3)
            rep["writer_threads"] = args.writer_threads
            print(json.dumps(rep), flush=True)


if __name__ == "__main__":
    main()
