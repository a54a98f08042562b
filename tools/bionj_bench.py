"""BIONJ on the host against the device, and the constant BIONJ_DEVICE_MIN.

    python tools/bionj_bench.py [--sizes 128,256,512,1024,2048] [--repeats 3] [--out profiles/bionj_bench.txt]

Per N: random float32 distances in (0.01, 3), one source.  host = hostio.bionj_newick (the serial bodies + the text, what
a writer thread runs); device = Engine.bionj_joins + hostio.newick_of_joins (what the GPU thread and then a writer thread
run).  The two texts are compared byte for byte BEFORE anything is timed; then the best of `repeats` of each,
alternating, in this one process.  BIONJ_DEVICE_MIN is the smallest of the sizes at which device <= host / 2 (the device
side occupies the GPU thread, the host side overlaps the next launch), never below 201.  The device's time per join
stands beside neighbour joining's of the same distances (Engine.nj_joins, profiles/nj_bench.txt)."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from phyloformer_amd import hostio  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512,1024,2048")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    lines = [f"# tools/bionj_bench.py --sizes {args.sizes} --repeats {args.repeats}",
             "# host = hostio.bionj_newick; device = Engine.bionj_joins + hostio.newick_of_joins (of which: the formatter); "
             "texts compared byte for byte before timing; best of the repeats, alternating; us_per_join = the device's "
             "joins alone / (N - 3), nj_us_per_join = Engine.nj_joins of the same distances",
             f"{'N':>6} {'host_ms':>10} {'device_ms':>10} {'format_ms':>10} {'host/device':>12} {'us_per_join':>12} {'nj_us_per_join':>15}  same_bytes"]
    chosen = None
    with Engine(load_weights(os.path.join(REPO, "models", "pf.ckpt")), 0) as e:
        info = e.device_info()
        lines.insert(1, f"# {info['name']}, kernel_hash {e.build_info().get('kernel_hash')}")
        e.bionj_joins(np.full(3, 1.0, np.float32))                   # (first-call costs are not what is compared)
        e.nj_joins(np.full(3, 1.0, np.float32))
        for n in sizes:
            preds = np.random.default_rng(n).uniform(0.01, 3.0, size=n * (n - 1) // 2).astype(np.float32)
            ids = [f"s{k}" for k in range(n)]
            want = hostio.bionj_newick(preds, ids)
            slots, lengths, flag = e.bionj_joins(preds)
            same = (not flag) and hostio.newick_of_joins(slots, lengths, ids) == want
            host, dev, fmt, nj = [], [], [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                hostio.bionj_newick(preds, ids)
                t1 = time.perf_counter()
                slots, lengths, flag = e.bionj_joins(preds)
                t2 = time.perf_counter()
                hostio.newick_of_joins(slots, lengths, ids)
                t3 = time.perf_counter()
                e.nj_joins(preds)
                t4 = time.perf_counter()
                host.append(t1 - t0), dev.append(t3 - t1), fmt.append(t3 - t2), nj.append(t4 - t3)
            h, d, f, j = min(host) * 1e3, min(dev) * 1e3, min(fmt) * 1e3, min(nj) * 1e3
            if chosen is None and same and n >= 201 and d <= h / 2:
                chosen = n
            lines.append(f"{n:>6} {h:>10.2f} {d:>10.2f} {f:>10.2f} {h / d:>12.2f} {(d - f) * 1e3 / (n - 3):>12.1f} {j * 1e3 / (n - 3):>15.1f}  {same}")
            print(lines[-1], flush=True)
    lines.append(f"BIONJ_DEVICE_MIN = {chosen if chosen is not None else 'none of these sizes qualifies'}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
