#!/usr/bin/env python3
"""Option site_dedup 1 against 0, alternated, on one engine: what walking distinct columns only buys and costs.

    python tools/site_dedup_compare.py [--repeats 4] [--steps 10] [--batch 16] [--n-seqs 60] [--n-sites 500]

Two batches of the headline shape, device-resident like bench.py's:
  distinct   every column of every alignment different (random residues, repeats redrawn): the worst case - the map is
             the identity whatever the option says, so the option can only cost (k_site_classes' comparisons, the
             indirect reads of k_colstats / k_colfin / k_main);
  bench      bench.py's own data, simulate_batch(8, N, L, seed=3) tiled to the batch: conserved columns as simulated.
Per batch and repeat: the rate of `steps` forwards (two streams, the default schedule) with the option at 1 and at 0,
then - one stream, HIP events around every launch - the milliseconds per launch of k_site_classes, k_colstats, k_colfin
and k_main.  Every repeat is printed: the spread of the repeats is what a difference has to be read against.  The
distances of both settings are compared bit for bit.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ("site_classes", "colstats", "colfin", "main")


def distinct_batch(B, N, L, seed=11):
    """uint8[B, N, L] of random residues in which no alignment has two equal columns."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 22, (B, N, L)).astype(np.uint8)
    for b in range(B):
        while True:
            _, first = np.unique(idx[b].T, axis=0, return_index=True)
            dup = np.setdiff1d(np.arange(L), first)
            if not len(dup):
                break
            idx[b][:, dup] = rng.integers(0, 22, (N, len(dup)))
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--n-seqs", type=int, default=60)
    ap.add_argument("--n-sites", type=int, default=500)
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.weights import load_weights
    B, N, L = args.batch, args.n_seqs, args.n_sites
    P = N * (N - 1) // 2
    base = simulate_batch(min(B, 8), N, L, seed=3)
    batches = {"distinct": distinct_batch(B, N, L), "bench": np.ascontiguousarray(base[np.arange(B) % base.shape[0]])}
    e = Engine(load_weights(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models", "pf.ckpt")), 0)
    info = e.device_info()
    print(f"# {info['name'].strip()}, kernel_hash {e.build_info().get('kernel_hash')}, {B} x {N} x {L}, {args.steps} steps per figure")
    d_idx, d_out = e.malloc(B * N * L), e.malloc(B * P * 4)
    for name, idx in batches.items():
        e.set_option("site_dedup", 1)
        _, ucount = e.site_classes(idx)
        print(f"## {name}: distinct columns per alignment {ucount.tolist()}, "
              f"{int(sum((u + 31) // 32 for u in ucount))} of {B * ((L + 31) // 32)} chunks of 32 sites")
        e.h2d(d_idx, idx)
        outs = {}
        for rep in range(args.repeats):
            for dedup in (1, 0):
                e.set_option("site_dedup", dedup)
                e.set_option("two_streams", 1)
                e.forward_device(d_idx, B, N, L, d_out)
                e.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    e.forward_device(d_idx, B, N, L, d_out)
                e.synchronize()
                dt = time.perf_counter() - t0
                res = np.empty((B, P), np.float32)
                e.d2h(res, d_out)
                outs[dedup] = res
                e.set_option("two_streams", 0)
                e.set_option("profile", 1)
                e.profile_reset()
                for _ in range(3):
                    e.forward_device(d_idx, B, N, L, d_out)
                e.synchronize()
                per = {k: e.profile_get(k) for k in KERNELS}
                e.set_option("profile", 0)
                ms = "  ".join(f"{k} {v[1] / max(v[0], 1):.4f}" for k, v in per.items())
                print(f"repeat {rep} site_dedup {dedup}: {B * args.steps / dt:8.2f} alignments/s  {dt / args.steps * 1e3:7.3f} ms/step | ms per launch, one stream: {ms}",
                      flush=True)
        print(f"distances bit-identical, site_dedup 1 against 0: {np.array_equal(outs[1].view(np.uint32), outs[0].view(np.uint32))}")
    e.free(d_idx)
    e.free(d_out)
    e.close()


if __name__ == "__main__":
    main()
