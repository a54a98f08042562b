"""split supports on the host against the device, and the constant SUPPORT_DEVICE_MIN.

    python tools/support_bench.py [--sizes 50,200,1024,4096] [--replicates 100] [--repeats 3] [--out profiles/support_bench.txt]
    python tools/support_bench.py --transfers [--cutoff 100] ... [--out profiles/transfer_bench.txt]      (section 27)

Per N: one source, a reference and R replicate join tables of random joins (the work does not depend on the trees: every
reference split meets every replicate split, word by word).  host = hostio.join_supports_host (the serial twin, what a
writer thread runs); device = Engine.join_supports (what the GPU thread runs: tables up, three kernels per chunk, results
down).  The results are compared for equality BEFORE anything is timed; then the best of `repeats` of each, alternating,
in this one process (a host run of more than 10 s is timed once).  SUPPORT_DEVICE_MIN is the smallest of the sizes at which
device <= host / 2 (the device side occupies the GPU thread, the host side overlaps the next launch).  Every row is
printed, and appended to --out, as soon as it is measured.

--transfers: the same for the per-taxon transfer counts and TRANSFER_DEVICE_MIN - host = hostio.join_transfers_host,
device = Engine.join_transfers, both with branch_moves as the CLI asks for them, at --cutoff percent (default 100: every
pair is used, the most work for k_sup_moves)."""
import argparse
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from phyloformer_amd import hostio  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402


def random_tables(n: int, count: int, seed: int) -> np.ndarray:
    """``int32 [count][2 (n - 3) + 3]``: valid join tables of random joins."""
    rng = random.Random(seed)
    out = np.zeros((count, 2 * (n - 3) + 3), dtype=np.int32)
    for k in range(count):
        alive = list(range(n))
        row = []
        for _ in range(n - 3):
            i = rng.randrange(len(alive))
            alive[i], alive[-1] = alive[-1], alive[i]
            b = alive.pop()
            j = rng.randrange(len(alive))
            a = alive[j]
            row += [min(a, b), max(a, b)]
            alive[j] = min(a, b)                                # (the new cluster takes the lower slot)
        out[k] = row + sorted(alive)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50,200,1024,4096")
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--transfers", action="store_true")
    ap.add_argument("--cutoff", type=int, default=100)
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
    name, constant = ("join_transfers", "TRANSFER_DEVICE_MIN") if args.transfers else ("join_supports", "SUPPORT_DEVICE_MIN")
    more = (None, args.cutoff) if args.transfers else ()

    def host_run(ref, reps):
        return getattr(hostio, name + "_host")(ref, reps, *more)
    with Engine(load_weights(os.path.join(REPO, "models", "pf.ckpt")), 0) as e:
        info = e.device_info()
        emit(f"# tools/support_bench.py{f' --transfers --cutoff {args.cutoff}' if args.transfers else ''} --sizes {args.sizes} "
             f"--replicates {R} --repeats {args.repeats}")
        emit(f"# {info['name']}, kernel_hash {e.build_info().get('kernel_hash')}")
        emit(f"# host = hostio.{name}_host (serial); device = Engine.{name} (host arrays in, host arrays out); results "
             "compared for equality before timing; best of the repeats, alternating (a host run above 10 s: once)")
        emit(f"{'N':>6} {'R':>4} {'word_ops':>10} {'host_ms':>11} {'device_ms':>10} {'host/device':>12}  same")
        warm = random_tables(8, 3, 0)
        device_run = getattr(e, name)
        device_run(warm[0], warm[1:], *more)                        # (first-call costs are not what is compared)
        for n in sizes:
            tables = random_tables(n, R + 1, n)
            ref, reps = tables[0], tables[1:]
            t0 = time.perf_counter()
            want = host_run(ref, reps)
            first = time.perf_counter() - t0
            got = device_run(ref, reps, *more)
            same = all(np.array_equal(g, w) for g, w in zip(got, want))
            host, dev = [first], []
            for _ in range(args.repeats):
                if first <= 10.0:
                    t0 = time.perf_counter()
                    host_run(ref, reps)
                    host.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                device_run(ref, reps, *more)
                dev.append(time.perf_counter() - t0)
            h, d = min(host) * 1e3, min(dev) * 1e3
            if chosen is None and same and d <= h / 2:
                chosen = n
            ops = (n - 3) ** 2 * R * ((n + 63) // 64)
            emit(f"{n:>6} {R:>4} {ops:>10.2e} {h:>11.2f} {d:>10.2f} {h / d:>12.2f}  {same}")
    emit(f"{constant} = {chosen if chosen is not None else 'none of these sizes qualifies'}")


if __name__ == "__main__":
    main()
