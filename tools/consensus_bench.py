"""majority-rule consensus on the host against the device, and the constant CONSENSUS_DEVICE_MIN.

    python tools/consensus_bench.py [--sizes 50,200,1024,4096] [--replicates 100] [--repeats 3] [--out profiles/consensus_bench.txt]

Per N: one source of R replicate join tables with branch lengths: 70 % of them one tree of random joins, the others
unrelated trees of random joins - every split of the one tree is selected (M = N - 3: the ranking, the nesting and the
length sums at their largest) and the hash table holds the unrelated trees' splits beside them.  host =
hostio.join_consensus_host (the serial twin, what a writer thread runs); device = Engine.join_consensus (what the GPU
thread runs: tables and lengths up, nine kernels per chunk, results down).  The results are compared bit for bit BEFORE
anything is timed; then the best of `repeats` of each, alternating, in this one process (a host run of more than 10 s is
timed once).  CONSENSUS_DEVICE_MIN is the smallest of the sizes at which device <= host / 2 (the device side occupies the
GPU thread, the host side overlaps the next launch).  Every row is printed, and appended to --out, as soon as it is
measured."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from phyloformer_amd import hostio  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402
from support_bench import random_tables  # noqa: E402


def same_bits(got, want) -> bool:
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50,200,1024,4096")
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    R = args.replicates

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    chosen = None
    with Engine(load_weights(os.path.join(REPO, "models", "pf.ckpt")), 0) as e:
        info = e.device_info()
        emit(f"# tools/consensus_bench.py --sizes {args.sizes} --replicates {R} --repeats {args.repeats}")
        emit(f"# {info['name']}, kernel_hash {e.build_info().get('kernel_hash')}")
        emit("# host = hostio.join_consensus_host (serial); device = Engine.join_consensus (host arrays in, host arrays out); results "
             "compared bit for bit before timing; best of the repeats, alternating (a host run above 10 s: once)")
        emit(f"{'N':>6} {'R':>4} {'splits':>9} {'M':>6} {'host_ms':>11} {'device_ms':>10} {'host/device':>12}  same")
        warm = random_tables(8, 3, 0)
        e.join_consensus(warm, np.ones(warm.shape))                 # (first-call costs are not what is compared)
        for n in sizes:
            tables = random_tables(n, R, n)
            tables[:(7 * R) // 10] = tables[0]
            lengths = np.random.default_rng(n).random(tables.shape)
            t0 = time.perf_counter()
            want = hostio.join_consensus_host(tables, lengths)
            first = time.perf_counter() - t0
            got = e.join_consensus(tables, lengths)
            same = same_bits(got, want)
            host, dev = [first], []
            for _ in range(args.repeats):
                if first <= 10.0:
                    t0 = time.perf_counter()
                    hostio.join_consensus_host(tables, lengths)
                    host.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.join_consensus(tables, lengths)
                dev.append(time.perf_counter() - t0)
            h, d = min(host) * 1e3, min(dev) * 1e3
            if chosen is None and same and d <= h / 2:
                chosen = n
            emit(f"{n:>6} {R:>4} {R * (n - 3):>9} {int(want[0]):>6} {h:>11.2f} {d:>10.2f} {h / d:>12.2f}  {same}")
    emit(f"CONSENSUS_DEVICE_MIN = {chosen if chosen is not None else 'none of these sizes qualifies'}")


if __name__ == "__main__":
    main()
