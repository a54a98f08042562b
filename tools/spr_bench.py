"""balanced SPR refinement on the host against the device, the constant SPR_DEVICE_MIN, and the two
kernels of the pair table.

    python tools/spr_bench.py [--sizes 64,128,200,256,512,1024] [--host-max 256] [--pairs 256,1024,2048] [--repeats 3]
                              [--out profiles/spr_bench.txt]

Per N of --sizes: random float32 distances in (0.01, 3), one source.  host = hostio.spr_newick (NJ + search + the text,
what a writer thread runs); device = Engine.nj_joins + Engine.bme_spr + hostio.newick_of_joins (what the GPU thread and
then a writer thread run).  Up to --host-max the two texts and step counts are compared BEFORE anything is timed, then the
best of `repeats` of each, alternating, in this one process; above it the host (minutes to hours there) is not run and
the row says so.  SPR_DEVICE_MIN is the smallest of the sizes at which device <= host / 2.

Per N of --pairs: the pair table of one step (option "profile", the events around the kernel; option "spr_step_cap" = 1
ends the search after its first move), k_bme_pairs against k_bme_pairs_simple, alternating, every repeat printed so that
the spread shows; the two results are compared byte for byte.  Every row is printed, and appended to --out, as soon as
it is measured."""
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
    ap.add_argument("--sizes", default="64,128,200,256,512,1024")
    ap.add_argument("--host-max", type=int, default=256)
    ap.add_argument("--pairs", default="256,1024,2048")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",") if s]
    pairs = [int(s) for s in args.pairs.split(",") if s]

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def inputs(n):
        return np.random.default_rng(n).uniform(0.01, 3.0, size=n * (n - 1) // 2).astype(np.float32), [f"s{k}" for k in range(n)]

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    chosen = None
    with Engine(load_weights(os.path.join(REPO, "models", "pf.ckpt")), 0) as e:
        info = e.device_info()
        emit(f"# tools/spr_bench.py --sizes {args.sizes} --host-max {args.host_max} --pairs {args.pairs} --repeats {args.repeats}")
        emit(f"# {info['name']}, kernel_hash {e.build_info().get('kernel_hash')}")
        warm = np.full(3, 1.0, np.float32)
        e.bme_spr(warm, e.nj_joins(warm)[0])                        # (first-call costs are not what is compared)
        emit("# pair table of one step, ms per call: k_bme_pairs (tiled) against k_bme_pairs_simple, every repeat")
        emit(f"{'N':>6} {'tiled_ms':>30} {'simple_ms':>30} {'simple/tiled':>13}  same_bytes")
        e.set_option("spr_step_cap", 1)
        e.set_option("profile", 1)
        for n in pairs:
            preds, _ids = inputs(n)
            start = e.nj_joins(preds)[0]
            ms, outs = {0: [], 1: []}, {}
            for _ in range(args.repeats):
                for simple in (0, 1):
                    e.set_option("spr_pairs_simple", simple)
                    e.profile_reset()
                    outs[simple] = e.bme_spr(preds, start)
                    calls, total = e.profile_get("bme_pairs")
                    ms[simple].append(total / max(calls, 1))
            same = all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
                       for a, b in zip(outs[0], outs[1]))
            fmt = lambda v: " ".join(f"{x:.3f}" for x in v)
            emit(f"{n:>6} {fmt(ms[0]):>30} {fmt(ms[1]):>30} {min(ms[1]) / min(ms[0]):>13.2f}  {same}")
        e.set_option("spr_pairs_simple", 0)
        e.set_option("profile", 0)
        e.set_option("spr_step_cap", 0)
        emit("# host = hostio.spr_newick; device = Engine.nj_joins + Engine.bme_spr + hostio.newick_of_joins (of which: nj_joins, "
             "the formatter); texts and steps compared before timing; best of the repeats, alternating")
        emit(f"{'N':>6} {'steps':>6} {'host_ms':>12} {'device_ms':>10} {'nj_ms':>9} {'format_ms':>10} {'host/device':>12}  same_bytes")
        for n in sizes:
            preds, ids = inputs(n)
            with_host = n <= args.host_max
            start, _l, flag = e.nj_joins(preds)
            slots, lengths, steps, _length, status = e.bme_spr(preds, start)
            same = "not compared"
            if with_host:
                want, host_steps = hostio.spr_newick(preds, ids, with_steps=True)
                same = (not flag) and status == 0 and int(steps) == host_steps and hostio.newick_of_joins(slots, lengths, ids) == want
            host, dev, njt, fmt = [], [], [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                if with_host:
                    hostio.spr_newick(preds, ids)
                t1 = time.perf_counter()
                start, _l, flag = e.nj_joins(preds)
                t2 = time.perf_counter()
                slots, lengths, steps, _length, status = e.bme_spr(preds, start)
                t3 = time.perf_counter()
                hostio.newick_of_joins(slots, lengths, ids)
                t4 = time.perf_counter()
                host.append(t1 - t0), dev.append(t4 - t1), njt.append(t2 - t1), fmt.append(t4 - t3)
            h, d, j, f = min(host) * 1e3, min(dev) * 1e3, min(njt) * 1e3, min(fmt) * 1e3
            if chosen is None and same is True and d <= h / 2:
                chosen = n
            if with_host:
                emit(f"{n:>6} {int(steps):>6} {h:>12.2f} {d:>10.2f} {j:>9.2f} {f:>10.2f} {h / d:>12.2f}  {same}")
            else:
                emit(f"{n:>6} {int(steps):>6} {'not measured':>12} {d:>10.2f} {j:>9.2f} {f:>10.2f} {'-':>12}  {same}")
    emit(f"SPR_DEVICE_MIN = {chosen if chosen is not None else 'none of these sizes qualifies'}")


if __name__ == "__main__":
    main()
