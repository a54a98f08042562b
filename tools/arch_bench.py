#!/usr/bin/env python3
"""Alignments per second of the generic float64 path (csrc/pf_generic.hip.h) at 60 x 500 and 20 x 200, for the shipped
(64, 4) checkpoint forced onto it (option "generic" = 1) and for random 6-block models of (32, 2), (128, 8), (256, 4).
One JSON line per (architecture, shape).  GPU only.

    python tools/arch_bench.py [--seconds 3] [--only 128,8]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0, help="timed seconds per case (after one warm-up batch)")
    ap.add_argument("--only", default="", help="one architecture 'E,H' (64,4 = the shipped checkpoint forced)")
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.weights import load_weights, random_weights

    archs = [("pf (64, 4) forced", None), ("(32, 2)", (32, 2)), ("(128, 8)", (128, 8)), ("(256, 4)", (256, 4))]
    shapes = [(60, 500, 4), (20, 200, 16)]          # (N, L, batch)
    if args.only:
        want = tuple(int(v) for v in args.only.split(","))
        archs = [(n, a) for n, a in archs if (a or (64, 4)) == want]
    for name, arch in archs:
        w = load_weights(os.path.join(REPO, "models", "pf.ckpt")) if arch is None else \
            random_weights(0, n_blocks=6, n_heads=arch[1], embed_dim=arch[0], scale=2.0)
        with Engine(w, 0) as e:
            if arch is None:
                e.set_option("generic", 1)
            for (n, l, b) in shapes:
                idx = simulate_batch(b, n, l, seed=1)
                d_idx = e.malloc(idx.nbytes)
                d_out = e.malloc(b * n * (n - 1) // 2 * 4)
                e.h2d(d_idx, idx)
                e.forward_device(d_idx, b, n, l, d_out)
                e.synchronize()
                t0, reps = time.perf_counter(), 0
                while time.perf_counter() - t0 < args.seconds:
                    e.forward_device(d_idx, b, n, l, d_out)
                    e.synchronize()
                    reps += 1
                dt = time.perf_counter() - t0
                e.free(d_idx)
                e.free(d_out)
                print(json.dumps({"arch": name, "n_blocks": w.n_blocks, "shape": f"{n}x{l}", "batch": b,
                                  "alignments_per_s": round(reps * b / dt, 2), "ms_per_batch": round(1e3 * dt / reps, 2)}),
                      flush=True)


if __name__ == "__main__":
    main()
