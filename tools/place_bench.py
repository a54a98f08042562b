#!/usr/bin/env python3
"""Query placement against the separate calls it replaces.  Per shape M x L with Q queries and B
alignments per call, best of --repeat:

  place_ms        one pf_forward_place call (one upload, sets cut on the device, statistics reduced on the device)
  separate_ms     the Q + 2 pf_forward calls on host-built alignments of the same build - the whole, the backbone
                  (idx[:, :N]) and Q calls of the B sets place.join_query builds - and place.place_stats on the host
  host_build_ms   building those alignments on the host (part of separate_ms)
  place_over_separate

The results of both are compared bit for bit (distances) and to 1e-6 (statistics) before anything is timed.
One JSON line per shape.  GPU only.

    python tools/place_bench.py [--shapes 20x200x8x8,60x500x4x2] [--repeat 3]
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
    ap.add_argument("--shapes", default="20x200x8x8,60x500x4x2", help="MxLxQxB,... (B alignments per call)")
    args = ap.parse_args()
    from phyloformer_amd.engine import Engine
    from phyloformer_amd.msa_sim import simulate_batch
    from phyloformer_amd.place import join_query, place_stats
    from phyloformer_amd.weights import load_weights

    w = load_weights(os.path.join(REPO, "models", "pf.ckpt"))
    with Engine(w, 0) as e:
        for spec in args.shapes.split(","):
            M, L, Q, B = (int(v) for v in spec.split("x"))
            N = M - Q
            idx = simulate_batch(B, M, L, seed=1)
            build_s = [0.0]

            def separate():
                t0 = time.perf_counter()
                back = np.ascontiguousarray(idx[:, :N])
                joined = [join_query(idx, N, q) for q in range(Q)]
                build_s[0] = time.perf_counter() - t0
                whole, base = e.forward(idx), e.forward(back)
                sets = np.stack([e.forward(j) for j in joined], axis=1)
                return (whole, base) + place_stats(whole, base, sets, N, Q) + (sets,)

            got, want = e.forward_place(idx, Q, keep_sets=True), separate()
            for k in (0, 1, 2, 6):
                assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
            assert all(np.allclose(got[k], want[k], rtol=1e-6, atol=1e-12) for k in (3, 4, 5))
            t_place = timed(lambda: e.forward_place(idx, Q), args.repeat)
            t_sep = timed(separate, args.repeat)
            print(json.dumps({"shape": f"{M}x{L}", "Q": Q, "B": B, "place_ms": round(1e3 * t_place, 3),
                              "separate_ms": round(1e3 * t_sep, 3), "host_build_ms": round(1e3 * build_s[0], 3),
                              "place_over_separate": round(t_place / t_sep, 4),
                              "rechecked": e.rechecked_count()}), flush=True)


if __name__ == "__main__":
    main()
