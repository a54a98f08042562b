#!/usr/bin/env python3
"""pf_bootstrap_weighted against pf_bootstrap from the same build, and the cost of the weight read.

    python tools/weights_bench.py [--out FILE]

Best of 3 per figure, one process, one GPU.  Cases: R = 100 replicates at 20 x 200 (B = 8), 60 x 500 (B = 2) and
200 x 500 (B = 1), range re-check on (default) and off; the padded K / L of each case stands beside the time ratio -
the expectation is that the ratio follows it.  The per-kernel shares (pf_profile_get) of both calls follow each case.
Then pf_forward_weighted_device with unit weights against pf_forward_device at 60 x 500 batch 16: one float read per
token beside the 587 bytes a token moves.  Prints one JSON line per figure.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phyloformer_amd import weights_sites as ws  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.msa_sim import simulate_batch  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402

KERNELS = ("embed", "rowfin", "colstats", "colfin", "main", "precise", "resample", "gather", "weight_sums")


def best_of(fn, n=3):
    fn()                                           # warm-up: workspaces, first-touch
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def shares(e, fn):
    e.set_option("profile", 1)
    e.profile_reset()
    fn()
    out = {k: round(e.profile_get(k)[1], 3) for k in KERNELS if e.profile_get(k)[0]}
    e.set_option("profile", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--replicates", type=int, default=100)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []

    def emit(rec):
        text = json.dumps(rec)
        print(text, flush=True)
        lines.append(text)
    with Engine(load_weights(os.path.join(root, "models", "pf.ckpt")), 0) as e:
        R, seed = args.replicates, 1
        for (n, l, b) in [(20, 200, 8), (60, 500, 2), (200, 500, 1)]:
            idx = simulate_batch(b, n, l, seed=n + l)
            K = ws.boot_tables(l, R, seed)[0].shape[1]
            for recheck in (8, 0):
                e.set_option("recheck_above", recheck)
                t_plain = best_of(lambda: e.bootstrap(idx, R, seed))
                t_w = best_of(lambda: e.bootstrap_weighted(idx, R, seed))
                emit({"case": f"{n}x{l} B={b} R={R}", "recheck": bool(recheck), "bootstrap_s": round(t_plain, 5),
                      "bootstrap_weighted_s": round(t_w, 5), "ratio": round(t_w / t_plain, 4), "K": K, "K_over_L": round(K / l, 4)})
            e.set_option("recheck_above", 8)
            emit({"case": f"{n}x{l} B={b} R={R}", "kernel_ms_bootstrap": shares(e, lambda: e.bootstrap(idx, R, seed)),
                  "kernel_ms_bootstrap_weighted": shares(e, lambda: e.bootstrap_weighted(idx, R, seed))})
        B, N, L = 16, 60, 500
        P = N * (N - 1) // 2
        idx = simulate_batch(B, N, L, seed=5)
        ones = np.ones((B, L), np.float32)
        d_idx, d_w, d_out = e.malloc(idx.nbytes), e.malloc(ones.nbytes), e.malloc(B * P * 4)
        try:
            e.h2d(d_idx, idx)
            e.h2d(d_w, ones)

            def plain():
                for _ in range(5):
                    e.forward_device(d_idx, B, N, L, d_out)
                e.synchronize()

            def weighted():
                for _ in range(5):
                    e.forward_weighted_device(d_idx, B, N, L, d_w, d_out)
                e.synchronize()
            t_p, t_w = best_of(plain) / 5, best_of(weighted) / 5
            emit({"case": "60x500 batch 16, device-resident", "forward_device_s": round(t_p, 6),
                  "forward_weighted_device_s": round(t_w, 6), "ratio": round(t_w / t_p, 4)})
        finally:
            for p in (d_idx, d_w, d_out):
                e.free(p)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
