"""tree rooting on the host against the device, for NJ tables, caterpillars and balanced tables.

    python tools/root_bench.py [--sizes 20,60,200,255,512,1024,2048,4096,8192] [--tables nj,caterpillar,balanced]
                               [--host-max 2048] [--repeats 3] [--no-host] [--out profiles/root_bench.txt]

Per N and kind of table: the NJ table is Engine.nj_joins' of random float32 distances in (0.01, 3), with its own lengths; the
caterpillar is bme.caterpillar_slots, the balanced table joins neighbouring slots in rounds, both with random lengths in
(-0.1, 0.9).  host = hostio.tree_root_host, once, host clock; above --host-max sequences it is skipped (the twin is O(N^3): a
single run at 4,096 passes a minute).  device = pf_tree_root_device on device arrays, between two HIP events on the handle's
stream after a warm-up call of the same shape: best and worst of `repeats`.  engine = Engine.tree_root on host arrays (staging,
one synchronisation), host clock, best of `repeats`: what the CLI's GPU thread pays, and what root.ROOT_DEVICE_MIN is read from.
Every line that ran both asserts that the device's arrays equal the host's, bit for bit.  The last line names the smallest size
from which the engine call is ahead of the twin for every table (255 is the host route's cost just below NJ's own device
threshold and does not count)."""
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
from phyloformer_amd import root as R  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402


def table_of(e, kind: str, n: int, rng):
    """``(slots int32 [1, 1, T], lengths float64 [1, 1, T])``."""
    if kind == "nj":
        preds = rng.uniform(0.01, 3.0, size=(1, n * (n - 1) // 2)).astype(np.float32)
        slots, lengths, flag = e.nj_joins(preds)
        assert not np.asarray(flag).any()
        return np.ascontiguousarray(slots[:, None]), np.ascontiguousarray(lengths[:, None])
    one = bme.caterpillar_slots(n) if kind == "caterpillar" else balanced_slots(n)
    return (np.ascontiguousarray(one.astype(np.int32)[None, None]), rng.uniform(-0.1, 0.9, size=(1, 1, F.table_len(n))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,60,200,255,512,1024,2048,4096,8192")
    ap.add_argument("--tables", default="nj,caterpillar,balanced")
    ap.add_argument("--host-max", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="the device alone (under a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",") if s]
    kinds = args.tables.split(",")
    lines = [f"# tools/root_bench.py --sizes {args.sizes} --tables {args.tables} --host-max {args.host_max} --repeats {args.repeats}",
             "# host = hostio.tree_root_host, once (host clock; '-': skipped above --host-max, a single run would pass a minute); device = "
             "pf_tree_root_device between HIP events on the handle's stream, warmed up, best / worst of the repeats; engine_ms = "
             "Engine.tree_root on host arrays (host clock, best); same = device arrays == host arrays (asserted)",
             f"{'N':>6} {'table':>12} {'host_ms':>12} {'device_ms':>10} {'worst_ms':>10} {'engine_ms':>10} {'host/device':>12} "
             f"{'host/engine':>12}  same"]
    ahead = {}
    with Engine(load_weights(os.path.join(REPO, "models", "pf.ckpt")), 0) as e:
        lines.insert(1, f"# {e.device_info()['name']}")
        stream = C.c_void_p()
        e._check(e._lib.pf_get_stream(e._h, C.byref(stream)))
        ev = Events(stream.value)
        for n in sizes:
            for kind in kinds:
                slots, lengths = table_of(e, kind, n, np.random.default_rng(n + 7))
                width = F.table_len(n)
                out = (np.empty((1, 1, width)), np.empty((1, 1, width)), np.empty((1, 1, R.MID)), np.empty((1, 1), np.uint8))
                try:                                     # (the largest size runs if the memory allows)
                    e.tree_root(slots, lengths)
                except (MemoryError, RuntimeError) as err:
                    lines.append(f"# N = {n}, {kind}: not run ({err})")
                    print(lines[-1], flush=True)
                    continue
                bufs = [e.malloc(a.nbytes) for a in (slots, lengths, *out)]
                for host, dev in zip((slots, lengths), bufs):
                    e.h2d(dev, host)
                call = lambda: e.tree_root_device(*bufs[:2], 1, 1, n, *bufs[2:])   # noqa: E731
                call()
                e.synchronize()
                ms = [ev.time_ms(call) for _ in range(args.repeats)]
                for host, dev in zip(out, bufs[2:]):
                    e.d2h(host, dev)
                e.synchronize()
                for p in bufs:
                    e.free(p)
                staged = e.tree_root(slots, lengths)
                engine_ms = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    e.tree_root(slots, lengths)
                    engine_ms.append((time.perf_counter() - t0) * 1e3)
                assert all(g.tobytes() == w.tobytes() for g, w in zip(out, staged)) and not staged[3].any(), (n, kind)
                host, same, r1, r2 = "-", "-", "-", "-"
                if not args.no_host and n <= args.host_max:
                    t0 = time.perf_counter()
                    want = hostio.tree_root_host(slots, lengths)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    host, r1, r2 = f"{host_ms:.3f}", f"{host_ms / min(ms):.1f}", f"{host_ms / min(engine_ms):.1f}"
                    for got in (out, staged):
                        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (n, kind)
                    same = "True"
                    ahead.setdefault(n, []).append(min(engine_ms) < host_ms)
                lines.append(f"{n:>6} {kind:>12} {host:>12} {min(ms):>10.3f} {max(ms):>10.3f} {min(engine_ms):>10.3f} {r1:>12} {r2:>12}  {same}")
                print(lines[-1], flush=True)
    measured = [n for n in sorted(ahead) if n != 255]
    first = next((n for k, n in enumerate(measured) if all(all(ahead[x]) for x in measured[k:])), None)
    lines.append(f"# the engine call is ahead of the twin for every table from N = {first} on: root.ROOT_DEVICE_MIN")
    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
