"""the tree fit on the host against the device, for NJ tables, caterpillars and balanced tables.

    python tools/fit_bench.py [--sizes 20,60,200,512,1024,2048,4096] [--tables nj,caterpillar,balanced] [--batch 256]
                              [--batch-max 200] [--repeats 3] [--out profiles/fit_bench.txt]

Per N and kind of table: random float32 distances in (0.01, 3); the NJ table is Engine.nj_joins' of them, the caterpillar
(bme.caterpillar_slots) and the balanced table (joins of neighbouring slots in rounds) carry random lengths.  host = hostio.
tree_fit_host, once, host clock.  device = pf_tree_fit_device on device arrays with the patristic array, between two HIP events
on the handle's stream after a warm-up call of the same shape: best and worst of `repeats`; rows_ms = the same without the
patristic array (the distances stay in the workspace).  engine = Engine.tree_fit on host arrays (staging, one synchronisation),
host clock, best of `repeats`: what the CLI's GPU thread pays.  Up to --batch-max sequences the line is repeated for B = --batch
sources, a launch of the CLI.  same = the device's arrays equal the host's, bit for bit."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from phyloformer_amd import bme, hostio  # noqa: E402
from phyloformer_amd import fit as F  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402


class Events:
    """Two HIP events on a stream."""

    def __init__(self, stream):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for ev in (self.a, self.b):
            self.check(self.hip.hipEventCreate(C.byref(ev)))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def time_ms(self, enqueue) -> float:
        self.check(self.hip.hipEventRecord(self.a, self.stream))
        enqueue()
        self.check(self.hip.hipEventRecord(self.b, self.stream))
        self.check(self.hip.hipEventSynchronize(self.b))
        ms = C.c_float()
        self.check(self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return float(ms.value)


def balanced_slots(n: int) -> np.ndarray:
    """Joins of neighbouring live slots in rounds until three are left: a leaf is about log2 n nodes below the last node."""
    live, table = list(range(n)), []
    while len(live) > 3:
        nxt, k, count = [], 0, len(live)
        while k < len(live):
            if k + 1 < len(live) and count > 3:
                table += [live[k], live[k + 1]]
                nxt.append(live[k])
                k, count = k + 2, count - 1
            else:
                nxt.append(live[k])
                k += 1
        live = nxt
    return np.array(table + live, dtype=np.int32)


def tables_of(e, kind: str, preds: np.ndarray, n: int, rng):
    b = len(preds)
    if kind == "nj":
        slots, lengths, flag = e.nj_joins(preds)
        assert not np.asarray(flag).any()
        return np.ascontiguousarray(slots[:, None]), np.ascontiguousarray(lengths[:, None])
    one = bme.caterpillar_slots(n) if kind == "caterpillar" else balanced_slots(n)
    slots = np.ascontiguousarray(np.broadcast_to(one.astype(np.int32), (b, 1, F.table_len(n))))
    return slots, rng.uniform(0.01, 1.0, size=slots.shape)


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
    lines = [f"# tools/fit_bench.py --sizes {args.sizes} --tables {args.tables} --batch {args.batch} --batch-max {args.batch_max} "
             f"--repeats {args.repeats}",
             "# host = hostio.tree_fit_host, once (host clock); device = pf_tree_fit_device with the patristic array between HIP "
             "events on the handle's stream, warmed up, best / worst of the repeats; rows_ms = the same without the patristic "
             "array; engine_ms = Engine.tree_fit on host arrays (host clock, best); same = device arrays == host arrays",
             f"{'N':>6} {'B':>5} {'table':>12} {'host_ms':>12} {'device_ms':>10} {'worst_ms':>10} {'rows_ms':>10} {'engine_ms':>10} "
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
                    pairs = n * (n - 1) // 2
                    preds = rng.uniform(0.01, 3.0, size=(b, pairs)).astype(np.float32)
                    slots, lengths = tables_of(e, kind, preds, n, rng)
                    out = (np.empty((b, 1, pairs)), np.empty((b, 1, n, F.COLS)), np.empty((b, 1, n), np.int32), np.empty((b, 1), np.uint8))
                    bufs = [e.malloc(a.nbytes) for a in (preds, slots, lengths, *out)]
                    for host, dev in zip((preds, slots, lengths), bufs):
                        e.h2d(dev, host)
                    call = lambda keep=True: e.tree_fit_device(*bufs[:3], b, 1, n, bufs[3] if keep else 0, *bufs[4:])   # noqa: E731
                    call()
                    e.synchronize()
                    ms = [ev.time_ms(call) for _ in range(args.repeats)]
                    for host, dev in zip(out, bufs[3:]):
                        e.d2h(host, dev)
                    e.synchronize()
                    call(False)
                    e.synchronize()
                    rows_ms = [ev.time_ms(lambda: call(False)) for _ in range(args.repeats)]
                    for p in bufs:
                        e.free(p)
                    e.tree_fit(preds, slots, lengths)
                    engine_ms = []
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        e.tree_fit(preds, slots, lengths)
                        engine_ms.append((time.perf_counter() - t0) * 1e3)
                    host, same, r1, r2 = "-", "-", "-", "-"
                    if not args.no_host:
                        t0 = time.perf_counter()
                        want = hostio.tree_fit_host(preds, slots, lengths)
                        host_ms = (time.perf_counter() - t0) * 1e3
                        host, r1, r2 = f"{host_ms:.3f}", f"{host_ms / min(ms):.1f}", f"{host_ms / min(engine_ms):.1f}"
                        same = str(all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                                       for g, w in zip(out, want)))
                    lines.append(f"{n:>6} {b:>5} {kind:>12} {host:>12} {min(ms):>10.3f} {max(ms):>10.3f} {min(rows_ms):>10.3f} "
                                 f"{min(engine_ms):>10.3f} {r1:>12} {r2:>12}  {same}")
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
