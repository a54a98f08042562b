#!/usr/bin/env python3
"""Site-window scan rates.  Per shape (60 x 2000 W = 500 step = 250, 20 x 1000 W = 200 step = 100):

  windows_per_s          pf_forward_windows windows/s (host buffers in and out, windows cut on the device, re-check)
  cut_fwd_windows_per_s  the way without the entry point: pf_forward on the host-cut [B * S][N][W] batch, upload of
                         every window included (the cut itself, numpy on the host, is timed apart: host_cut_ms)
  windows_over_cut_fwd   time of pf_forward_windows / time of pf_forward on the host-cut batch (< 1: faster)
  upload_bytes           source bytes pf_forward_windows uploads / window bytes the host-cut batch uploads
  gather_ms, gather_share  k_gather_sites' time and share of the GPU time of one call (option "profile" = 1: HIP events)

Best of --repeat.  One JSON line per shape.  GPU only.  ``--trace N`` only issues N pf_forward_windows calls per
shape and prints nothing else: the workload of a ``rocprofv3 --kernel-trace --stats`` run of its own.

    python tools/windows_bench.py [--repeat 3] [--shapes 60x2000x500x250x2,20x1000x200x100x8]
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
    ap.add_argument("--shapes", default="60x2000x500x250x2,20x1000x200x100x8",
                    help="NxLxWxSTEPxB,... (B source alignments per call)")
    ap.add_argument("--trace", type=int, default=0, help="only issue this many pf_forward_windows calls per shape")
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.weights import load_weights
    from phyloformer_amd.windows import cut_sites, window_sites

    names = ["embed", "rowfin", "colstats", "colfin", "main", "allreduce", "precise", "generic", "resample", "gather"]
    w = load_weights(os.path.join(REPO, "models", "pf.ckpt"))
    with Engine(w, 0) as e:
        for spec in args.shapes.split(","):
            N, L, W, step, B = (int(v) for v in spec.split("x"))
            idx = simulate_batch(B, N, L, seed=1)
            if args.trace:
                for _ in range(args.trace):
                    e.forward_windows(idx, W, step)
                continue
            sites = window_sites(L, W, step)
            S = len(sites)
            rep = {"shape": f"{N}x{L}", "W": W, "step": step, "B": B, "S": S}
            t_win = timed(lambda: e.forward_windows(idx, W, step), args.repeat)
            rep["windows_per_s"] = round(B * S / t_win, 1)
            rep["host_cut_ms"] = round(1e3 * timed(lambda: cut_sites(idx, sites), args.repeat), 3)
            cut = cut_sites(idx, sites).reshape(B * S, N, W)
            t_cut = timed(lambda: e.forward(cut), args.repeat)
            rep["cut_fwd_windows_per_s"] = round(B * S / t_cut, 1)
            rep["windows_over_cut_fwd"] = round(t_win / t_cut, 4)
            rep["upload_bytes"] = [int(idx.nbytes), int(cut.nbytes)]
            got = e.forward_windows(idx, W, step)
            rep["bit_identical"] = bool(np.array_equal(got.reshape(B * S, -1).view(np.uint32), e.forward(cut).view(np.uint32)))
            e.set_option("profile", 1)
            e.profile_reset()
            e.forward_windows(idx, W, step)
            ms = {k: e.profile_get(k)[1] for k in names}
            e.set_option("profile", 0)
            rep["gather_ms"] = round(ms["gather"], 4)
            rep["gather_share"] = round(ms["gather"] / max(1e-9, sum(ms.values())), 5)
            print(json.dumps(rep), flush=True)


if __name__ == "__main__":
    main()
