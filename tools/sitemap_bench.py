#!/usr/bin/env python3
"""What the site map costs.  Per shape (60 x 500 batch 16, 20 x 200 batch 64, 20 x 200 batch 1):

  forward_device_ms        pf_forward_device, device buffers in and out
  site_map_device_ms       pf_forward_site_map_device (the same forward, the last block also stores the map)
  map_device_over_forward  their ratio
  forward_ms               pf_forward, host buffers in and out
  site_profile_ms          pf_forward_site_profile (host buffers; the map stays on the device and is reduced there)
  site_map_ms              pf_forward_site_map (host buffers; the map is copied to the host: map_mbytes)
  profile_over_forward, map_over_forward   ratios to pf_forward
  site_moments_ms, site_moments_share      the reduction's time and share of the GPU time of one pf_forward_site_profile
                                           call (option "profile" = 1: HIP events)

Best of --repeat.  One JSON line per shape.  GPU only.

    python tools/sitemap_bench.py [--repeat 5] [--shapes 60x500x16,20x200x64,20x200x1]
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
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--shapes", default="60x500x16,20x200x64,20x200x1", help="NxLxB,...")
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.weights import load_weights

    names = ["embed", "rowfin", "colstats", "colfin", "main", "allreduce", "precise", "generic", "site_moments"]
    w = load_weights(os.path.join(REPO, "models", "pf.ckpt"))
    with Engine(w, 0) as e:
        for spec in args.shapes.split(","):
            N, L, B = (int(v) for v in spec.split("x"))
            P = N * (N - 1) // 2
            idx = simulate_batch(B, N, L, seed=1)
            d_idx, d_out, d_map = e.malloc(idx.nbytes), e.malloc(B * P * 4), e.malloc(B * P * L * 4)
            e.h2d(d_idx, idx)

            def fwd_dev():
                e.forward_device(d_idx, B, N, L, d_out)
                e.synchronize()

            def map_dev():
                e.forward_site_map_device(d_idx, B, N, L, d_out, d_map)
                e.synchronize()
            rep = {"shape": f"{N}x{L}", "B": B, "map_mbytes": round(B * P * L * 4 / 1e6, 2)}
            t_fd, t_md = timed(fwd_dev, args.repeat), timed(map_dev, args.repeat)
            rep["forward_device_ms"], rep["site_map_device_ms"] = round(1e3 * t_fd, 4), round(1e3 * t_md, 4)
            rep["map_device_over_forward"] = round(t_md / t_fd, 4)
            t_f = timed(lambda: e.forward(idx), args.repeat)
            t_p = timed(lambda: e.forward_site_profile(idx), args.repeat)
            t_m = timed(lambda: e.forward_site_map(idx), args.repeat)
            rep["forward_ms"], rep["site_profile_ms"], rep["site_map_ms"] = (round(1e3 * t, 4) for t in (t_f, t_p, t_m))
            rep["profile_over_forward"], rep["map_over_forward"] = round(t_p / t_f, 4), round(t_m / t_f, 4)
            e.set_option("profile", 1)
            e.profile_reset()
            got = e.forward_site_profile(idx)
            ms = {k: e.profile_get(k)[1] for k in names}
            e.set_option("profile", 0)
            rep["site_moments_ms"] = round(ms["site_moments"], 4)
            rep["site_moments_share"] = round(ms["site_moments"] / max(1e-9, sum(ms.values())), 5)
            rep["out_bit_identical"] = bool(np.array_equal(got[0].view(np.uint32), e.forward(idx).view(np.uint32)))
            for p in (d_idx, d_out, d_map):
                e.free(p)
            print(json.dumps(rep), flush=True)


if __name__ == "__main__":
    main()
