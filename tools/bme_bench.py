"""balanced NNI refinement on the host against the device, and the constant BME_DEVICE_MIN.

    python tools/bme_bench.py [--sizes 64,128,200,256,512,1024,2048] [--repeats 3] [--out profiles/bme_bench.txt]

Per N: random float32 distances in (0.01, 3), one source.  host = hostio.bme_newick (NJ + refinement + the text, what a
writer thread runs); device = Engine.nj_joins + Engine.bme_nni + hostio.newick_of_joins (what the GPU thread and then a
writer thread run).  The two texts are compared byte for byte BEFORE anything is timed; then the best of `repeats` of
each, alternating, in this one process.  BME_DEVICE_MIN is the smallest of the sizes at which device <= host / 2 (the
device side occupies the GPU thread, the host side overlaps the next launch).  Every row is printed, and appended to
--out, as soon as it is measured."""
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
    ap.add_argument("--sizes", default="64,128,200,256,512,1024,2048")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]

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
        emit(f"# tools/bme_bench.py --sizes {args.sizes} --repeats {args.repeats}")
        emit(f"# {info['name']}, kernel_hash {e.build_info().get('kernel_hash')}")
        emit("# host = hostio.bme_newick; device = Engine.nj_joins + Engine.bme_nni + hostio.newick_of_joins (of which: nj_joins, "
             "the formatter); texts compared byte for byte before timing; best of the repeats, alternating")
        emit(f"{'N':>6} {'steps':>6} {'host_ms':>11} {'device_ms':>10} {'nj_ms':>9} {'format_ms':>10} {'host/device':>12}  same_bytes")
        warm = np.full(3, 1.0, np.float32)
        e.bme_nni(warm, e.nj_joins(warm)[0])                        # (first-call costs are not what is compared)
        for n in sizes:
            preds = np.random.default_rng(n).uniform(0.01, 3.0, size=n * (n - 1) // 2).astype(np.float32)
            ids = [f"s{k}" for k in range(n)]
            want, host_steps = hostio.bme_newick(preds, ids, with_steps=True)
            start, _l, flag = e.nj_joins(preds)
            slots, lengths, steps, _length, status = e.bme_nni(preds, start)
            same = (not flag) and status == 0 and int(steps) == host_steps and hostio.newick_of_joins(slots, lengths, ids) == want
            host, dev, njt, fmt = [], [], [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                hostio.bme_newick(preds, ids)
                t1 = time.perf_counter()
                start, _l, flag = e.nj_joins(preds)
                t2 = time.perf_counter()
                slots, lengths, steps, _length, status = e.bme_nni(preds, start)
                t3 = time.perf_counter()
                hostio.newick_of_joins(slots, lengths, ids)
                t4 = time.perf_counter()
                host.append(t1 - t0), dev.append(t4 - t1), njt.append(t2 - t1), fmt.append(t4 - t3)
            h, d, j, f = min(host) * 1e3, min(dev) * 1e3, min(njt) * 1e3, min(fmt) * 1e3
            if chosen is None and same and d <= h / 2:
                chosen = n
            emit(f"{n:>6} {int(steps):>6} {h:>11.2f} {d:>10.2f} {j:>9.2f} {f:>10.2f} {h / d:>12.2f}  {same}")
    emit(f"BME_DEVICE_MIN = {chosen if chosen is not None else 'none of these sizes qualifies'}")


if __name__ == "__main__":
    main()
