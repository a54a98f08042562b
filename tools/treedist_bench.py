"""the tree distances on the host against the device, for identical trees, unrelated trees and 70 % one tree.

    python tools/treedist_bench.py [--sizes 20,60,200,512,1024,4096] [--trees 7,101] [--mixes identical,unrelated,seventy]
                                   [--repeats 3] [--no-host] [--out profiles/treedist_bench.txt]

Per N, K and mix: K valid join tables of random joins (identical: one table K times; unrelated: K tables; seventy: 70 % of
the trees are the first one, the others random) with gaussian lengths.  host = hostio.join_distances_host on the host clock,
best of `repeats` (once from N = 1,024 on).  device = pf_join_distances_device on device arrays, between two HIP events on the
handle's stream after a warm-up call of the same shape: best and worst of `repeats`.  engine = Engine.join_distances on host
arrays (staging, one synchronisation), host clock, best of `repeats`: what the CLI's GPU thread pays, and what
treedist.TREEDIST_DEVICE_MIN (K = 7) and TREEDIST_REPS_DEVICE_MIN (K = 101) are read from: the smallest measured N at which
engine_ms is at most half of host_ms in every mix.  The bits are compared before anything is timed."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from fit_bench import Events  # noqa: E402
from phyloformer_amd import hostio  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402


def random_table(n: int, rng) -> np.ndarray:
    """A valid join table of random joins."""
    out = np.zeros(2 * (n - 3) + 3, dtype=np.int32)
    alive = list(range(n))
    for t in range(n - 3):
        i, j = rng.choice(len(alive), size=2, replace=False).tolist()
        out[2 * t], out[2 * t + 1] = alive[i], alive[j]
        alive[j] = alive[-1]
        alive.pop()
    out[2 * (n - 3):] = alive
    return out


def tables_of(mix: str, n: int, k: int, rng) -> np.ndarray:
    first = random_table(n, rng)
    same = {"identical": k, "unrelated": 1, "seventy": max(1, (7 * k) // 10)}[mix]
    return np.stack([first] * same + [random_table(n, rng) for _ in range(k - same)])


def best_ms(call, repeats: int) -> float:
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,60,200,512,1024,4096")
    ap.add_argument("--trees", default="7,101")
    ap.add_argument("--mixes", default="identical,unrelated,seventy")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="the device alone (under a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# tools/treedist_bench.py --sizes {args.sizes} --trees {args.trees} --mixes {args.mixes} --repeats {args.repeats}",
             "# host = hostio.join_distances_host (host clock, best; once from N = 1024 on); device = pf_join_distances_device "
             "between HIP events on the handle's stream, warmed up, best / worst of the repeats; engine_ms = Engine.join_distances "
             "on host arrays (host clock, best); same = device arrays == host arrays (asserted before timing)",
             f"{'N':>6} {'K':>5} {'mix':>10} {'host_ms':>12} {'device_ms':>10} {'worst_ms':>10} {'engine_ms':>10} "
             f"{'host/device':>12} {'host/engine':>12}  same"]
    with Engine(load_weights(os.path.join(REPO, "models", "pf.ckpt")), 0) as e:
        lines.insert(1, f"# {e.device_info()['name']}")
        stream = C.c_void_p()
        e._check(e._lib.pf_get_stream(e._h, C.byref(stream)))
        ev = Events(stream.value)
        for n in (int(s) for s in args.sizes.split(",") if s):
            for k in (int(s) for s in args.trees.split(",") if s):
                for mix in args.mixes.split(","):
                    rng = np.random.default_rng(n + 7 * k)
                    slots = np.ascontiguousarray(tables_of(mix, n, k, rng)[None])
                    lengths = rng.standard_normal(slots.shape)
                    flag = np.zeros((1, k), dtype=np.uint8)
                    out = (np.empty((1, k, k), np.int32), np.empty((1, k, k)), np.empty((1, k, k)), np.empty(1, np.uint8))
                    bufs = [e.malloc(a.nbytes) for a in (slots, lengths, flag, *out)]
                    for host, dev in zip((slots, lengths, flag), bufs):
                        e.h2d(dev, host)
                    call = lambda: e.join_distances_device(*bufs[:3], 1, k, n, *bufs[3:])   # noqa: E731
                    call()
                    for host, dev in zip(out, bufs[3:]):
                        e.d2h(host, dev)
                    e.synchronize()
                    staged = e.join_distances(slots, lengths, flag)
                    host, same, r1, r2, host_ms = "-", "-", "-", "-", None
                    if not args.no_host:
                        t0 = time.perf_counter()
                        want = hostio.join_distances_host(slots, lengths, flag)
                        host_ms = (time.perf_counter() - t0) * 1e3
                        for got in (out, staged):
                            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (n, k, mix)
                        assert not want[3].any()
                        same = "True"
                        if n < 1024:
                            host_ms = min(host_ms, best_ms(lambda: hostio.join_distances_host(slots, lengths, flag), args.repeats - 1))
                    ms = [ev.time_ms(call) for _ in range(args.repeats)]
                    e.synchronize()
                    for p in bufs:
                        e.free(p)
                    engine_ms = best_ms(lambda: e.join_distances(slots, lengths, flag), args.repeats)
                    if host_ms is not None:
                        host, r1, r2 = f"{host_ms:.3f}", f"{host_ms / min(ms):.1f}", f"{host_ms / engine_ms:.1f}"
                    lines.append(f"{n:>6} {k:>5} {mix:>10} {host:>12} {min(ms):>10.3f} {max(ms):>10.3f} {engine_ms:>10.3f} "
                                 f"{r1:>12} {r2:>12}  {same}")
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
