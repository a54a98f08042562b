"""the least-squares branch lengths on the host against the device, for NJ tables, caterpillars and balanced
tables.

    python tools/ols_bench.py [--sizes 20,60,200,512,1024,2048,4096] [--tables nj,caterpillar,balanced] [--batch 256]
                              [--batch-max 200] [--repeats 3] [--out profiles/ols_bench.txt]

Per N and kind of table: random float32 distances in (0.01, 3); the NJ table is Engine.nj_joins' of them, the caterpillar is
bme.caterpillar_slots, the balanced table joins neighbouring slots in rounds.  host = hostio.tree_ols_host, once, host clock.
device = pf_tree_ols_device on device arrays, between two HIP events on the handle's stream after a warm-up call of the same
shape: best and worst of `repeats`.  engine = Engine.tree_ols on host arrays (staging, one synchronisation), host clock, best of
`repeats`: what the CLI's GPU thread pays, and what ols.OLS_DEVICE_MIN is read from (the B = 1 lines).  Up to --batch-max
sequences the line is repeated for B = --batch sources, a launch of the CLI.  Every line asserts that the device's arrays equal
the host's, bit for bit."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from fit_bench import Events, balanced_slots  # noqa: E402
from phyloformer_amd import bme, hostio  # noqa: E402
from phyloformer_amd import fit as F  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402


def slots_of(e, kind: str, preds: np.ndarray, n: int) -> np.ndarray:
    b = len(preds)
    if kind == "nj":
        slots, _lengths, flag = e.nj_joins(preds)
        assert not np.asarray(flag).any()
        return np.ascontiguousarray(slots[:, None])
    one = bme.caterpillar_slots(n) if kind == "caterpillar" else balanced_slots(n)
    return np.ascontiguousarray(np.broadcast_to(one.astype(np.int32), (b, 1, F.table_len(n))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,60,200,512,1024,2048,4096")
    ap.add_argument("--tables", default="nj,caterpillar,balanced")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batch-max", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="the device alone (under a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",") if s]
    lines = [f"# tools/ols_bench.py --sizes {args.sizes} --tables {args.tables} --batch {args.batch} --batch-max {args.batch_max} "
             f"--repeats {args.repeats}",
             "# host = hostio.tree_ols_host, once (host clock); device = pf_tree_ols_device between HIP events on the handle's "
             "stream, warmed up, best / worst of the repeats; engine_ms = Engine.tree_ols on host arrays (host clock, best); "
             "same = device arrays == host arrays (asserted)",
             f"{'N':>6} {'B':>5} {'table':>12} {'host_ms':>12} {'device_ms':>10} {'worst_ms':>10} {'engine_ms':>10} "
             f"{'host/device':>12} {'host/engine':>12}  same"]
    with Engine(load_weights(os.path.join(REPO, "models", "pf.ckpt")), 0) as e:
        lines.insert(1, f"# {e.device_info()['name']}")
        stream = C.c_void_p()
        e._check(e._lib.pf_get_stream(e._h, C.byref(stream)))
        ev = Events(stream.value)
        for n in sizes:
            for b in ([1, args.batch] if n <= args.batch_max else [1]):
                for kind in args.tables.split(","):
                    rng = np.random.default_rng(n + 7 * b)
                    preds = rng.uniform(0.01, 3.0, size=(b, n * (n - 1) // 2)).astype(np.float32)
                    slots = slots_of(e, kind, preds, n)
                    out = (np.empty((b, 1, F.table_len(n))), np.empty((b, 1), np.uint8))
                    bufs = [e.malloc(a.nbytes) for a in (preds, slots, *out)]
                    for host, dev in zip((preds, slots), bufs):
                        e.h2d(dev, host)
                    call = lambda: e.tree_ols_device(*bufs[:2], b, 1, n, *bufs[2:])   # noqa: E731
                    call()
                    e.synchronize()
                    ms = [ev.time_ms(call) for _ in range(args.repeats)]
                    for host, dev in zip(out, bufs[2:]):
                        e.d2h(host, dev)
                    e.synchronize()
                    for p in bufs:
                        e.free(p)
                    staged = e.tree_ols(preds, slots)
                    engine_ms = []
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        e.tree_ols(preds, slots)
                        engine_ms.append((time.perf_counter() - t0) * 1e3)
                    host, same, r1, r2 = "-", "-", "-", "-"
                    if not args.no_host:
                        t0 = time.perf_counter()
                        want = hostio.tree_ols_host(preds, slots)
                        host_ms = (time.perf_counter() - t0) * 1e3
                        host, r1, r2 = f"{host_ms:.3f}", f"{host_ms / min(ms):.1f}", f"{host_ms / min(engine_ms):.1f}"
                        for got in (out, staged):
                            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (n, b, kind)
                        assert not want[1].any()
                        same = "True"
                    lines.append(f"{n:>6} {b:>5} {kind:>12} {host:>12} {min(ms):>10.3f} {max(ms):>10.3f} {min(engine_ms):>10.3f} "
                                 f"{r1:>12} {r2:>12}  {same}")
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
