#!/usr/bin/env python3
"""Option main_dedup 1 (and 2) against 0, alternated, on one engine: what k_main's per-token work once per distinct
column buys and costs (the approach of tools/site_dedup_compare.py).

    python tools/main_dedup_compare.py [--repeats 4] [--steps 10] [--modes 1,0] [--batches distinct,bench] [--option main_dedup]

Two batches of the headline shape, device-resident like bench.py's:
  distinct   every column of every alignment different: the worst case - with option 1 every alignment stays on the
             fused launch and the compact and statistics launches of every block return at once, so the option can
             only cost (the plan kernel, two empty launches per block, the fused launch's alignment list);
  bench      bench.py's own data, simulate_batch(8, N, L, seed=3) tiled to the batch.
Per batch and repeat: the rate of `steps` forwards (two streams, the default schedule) with the option at each mode in
turn, then - one stream, one pair of HIP events around each block's k_main launches - the milliseconds per block.  Every
repeat is printed: the spread of the repeats is what a difference has to be read against.  The distances of all modes are
compared bit for bit.  `--modes 2,0` on one stream under `rocprofv3 --kernel-trace --stats` gives the times of the
compact, statistics and fused launches the threshold is derived from (profiles/main_dedup_threshold.txt).
`--option stats_dedup` alternates that option instead (main_dedup stays at its default): the split route's statistics by
k_row_stats against the statistics launch; on the `distinct` batch nothing is split and neither runs
(profiles/stats_dedup_compare.txt).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.site_dedup_compare import distinct_batch  # noqa: E402

KERNELS = ("site_classes", "colstats", "main")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--n-seqs", type=int, default=60)
    ap.add_argument("--n-sites", type=int, default=500)
    ap.add_argument("--modes", default="1,0")
    ap.add_argument("--batches", default="distinct,bench")
    ap.add_argument("--option", default="main_dedup", choices=["main_dedup", "stats_dedup"], help="the option the modes are values of")
    ap.add_argument("--one-stream-only", action="store_true", help="skip the two-stream rate (profiler runs)")
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.weights import load_weights
    B, N, L = args.batch, args.n_seqs, args.n_sites
    P = N * (N - 1) // 2
    modes = [int(m) for m in args.modes.split(",")]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = Engine(load_weights(os.path.join(root, "models", "pf.ckpt")), 0)
    print(f"# {e.device_info()['name'].strip()}, kernel_hash {e.build_info().get('kernel_hash')}, {B} x {N} x {L}, "
          f"{args.steps} steps per figure")
    d_idx, d_out = e.malloc(B * N * L), e.malloc(B * P * 4)
    for name in args.batches.split(","):
        if name == "distinct":
            idx = distinct_batch(B, N, L)
        else:
            base = simulate_batch(min(B, 8), N, L, seed=3)
            idx = np.ascontiguousarray(base[np.arange(B) % base.shape[0]])
        _, ucount = e.site_classes(idx)
        print(f"## {name}: distinct columns per alignment {ucount.tolist()}")
        e.h2d(d_idx, idx)
        outs = {}
        for rep in range(args.repeats):
            for mode in modes:
                e.set_option(args.option, mode)
                rate = ""
                if not args.one_stream_only:
                    e.set_option("two_streams", 1)
                    e.forward_device(d_idx, B, N, L, d_out)
                    e.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        e.forward_device(d_idx, B, N, L, d_out)
                    e.synchronize()
                    dt = time.perf_counter() - t0
                    rate = f"{B * args.steps / dt:8.2f} alignments/s  {dt / args.steps * 1e3:7.3f} ms/step | "
                e.set_option("two_streams", 0)
                e.set_option("profile", 1)
                e.profile_reset()
                for _ in range(3):
                    e.forward_device(d_idx, B, N, L, d_out)
                e.synchronize()
                per = {k: e.profile_get(k) for k in KERNELS}
                e.set_option("profile", 0)
                res = np.empty((B, P), np.float32)
                e.d2h(res, d_out)
                outs[mode] = res
                ms = "  ".join(f"{k} {v[1] / max(v[0], 1):.4f} (x{v[0] // 3})" for k, v in per.items())
                print(f"repeat {rep} {args.option} {mode}: {rate}ms per bracket, one stream: {ms}", flush=True)
        same = all(np.array_equal(outs[m].view(np.uint32), outs[modes[0]].view(np.uint32)) for m in modes)
        print(f"distances bit-identical across {args.option} {modes}: {same}")
    e.set_option(args.option, 1)
    e.free(d_idx)
    e.free(d_out)
    e.close()


if __name__ == "__main__":
    main()
