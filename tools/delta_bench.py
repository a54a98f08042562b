"""delta scores on the host against the device, and the device's rate of quartet evaluations.

    python tools/delta_bench.py [--sizes 20,60,200,512,1024] [--device-only 2048] [--repeats 3] [--out profiles/delta_bench.txt]

Per N: random float32 distances in (0.01, 3), one source, 20 bins.  host = hostio.delta_host (every quartet once,
serially), timed once with the host clock; from 512 sequences on it runs on --host-cap sequences only and is scaled by
the ratio of C(N, 4).  device = pf_delta_device on device arrays between two HIP events on the handle's stream, after a
warm-up call of the same shape, best and worst of `repeats`; the arrays are compared with the host's where the host ran
whole.  Gq/s = the quartets of a second; launches = what the launch bound cuts a call into; owner_ms = the design
without atomics on the pair sums (option "delta_atomic" = 0), timed the same way."""
import argparse
import ctypes as C
import os
import sys
import time
from math import comb

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from phyloformer_amd import hostio  # noqa: E402
from phyloformer_amd.engine import Engine  # noqa: E402
from phyloformer_amd.weights import load_weights  # noqa: E402

LAUNCH_EVALS = 1 << 35        # csrc/pf_delta.hip.h


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,60,200,512,1024")
    ap.add_argument("--device-only", default="2048")
    ap.add_argument("--host-cap", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [(int(s), True) for s in args.sizes.split(",") if s] + [(int(s), False) for s in args.device_only.split(",") if s]
    lines = [f"# tools/delta_bench.py --sizes {args.sizes} --device-only {args.device_only} --host-cap {args.host_cap} --repeats {args.repeats}",
             "# host = hostio.delta_host, once (host clock; '~': measured at --host-cap sequences, scaled by C(N, 4)); device = "
             "pf_delta_device between HIP events on the handle's stream, warmed up, best / worst of the repeats; Gq/s = C(N, 4) / device_ms; owner_ms = the same call under option delta_atomic = 0 "
             "(every quartet six times, no atomics on the pair sums), owner_same = its arrays equal the product's",
             f"{'N':>6} {'quartets':>14} {'host_ms':>12} {'device_ms':>10} {'worst_ms':>10} {'host/device':>12} {'Gq/s':>9} "
             f"{'launches':>9} {'ms/launch':>10} {'owner_ms':>10}  same  owner_same"]
    with Engine(load_weights(os.path.join(REPO, "models", "pf.ckpt")), 0) as e:
        lines.insert(1, f"# {e.device_info()['name']}")
        stream = C.c_void_p()
        e._check(e._lib.pf_get_stream(e._h, C.byref(stream)))
        ev = Events(stream.value)
        for n, with_host in sizes:
            pairs, k = n * (n - 1) // 2, args.bins
            preds = np.random.default_rng(n).uniform(0.01, 3.0, size=pairs).astype(np.float32)
            d_p, d_sum, d_hist, d_flag = e.malloc(4 * pairs), e.malloc(8 * pairs), e.malloc(8 * k), e.malloc(8)
            e.h2d(d_p, preds)
            call = lambda: e.delta_device(d_p, 1, n, k, d_sum, d_hist, d_flag)   # noqa: E731
            call()
            e.synchronize()
            ms = [ev.time_ms(call) for _ in range(args.repeats)]
            got = (np.empty(pairs, np.int64), np.empty(k, np.int64))
            e.d2h(got[0], d_sum), e.d2h(got[1], d_hist)
            # the design without atomics on the pair sums (option "delta_atomic" = 0): its own warm-up, the same repeats
            e.set_option("delta_atomic", 0)
            call()
            e.synchronize()
            owner_ms = [ev.time_ms(call) for _ in range(args.repeats)]
            e.set_option("delta_atomic", 1)
            alt = (np.empty(pairs, np.int64), np.empty(k, np.int64))
            e.d2h(alt[0], d_sum), e.d2h(alt[1], d_hist)
            owner_same = np.array_equal(alt[0], got[0]) and np.array_equal(alt[1], got[1])
            for p in (d_p, d_sum, d_hist, d_flag):
                e.free(p)
            host, same = "", "-"
            if with_host:
                m = min(n, args.host_cap)
                sub = preds if m == n else np.random.default_rng(m).uniform(0.01, 3.0, size=m * (m - 1) // 2).astype(np.float32)
                t0 = time.perf_counter()
                want = hostio.delta_host(sub)
                host_ms = (time.perf_counter() - t0) * 1e3 * comb(n, 4) / comb(m, 4)
                host = f"{'' if m == n else '~'}{host_ms:.2f}"
                if m == n:
                    same = str(np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))
            if got[1].sum() != comb(n, 4):
                same = "False"
            launches = -(-pairs // max(1, min(LAUNCH_EVALS // comb(n - 2, 2), 1 << 30)))
            ratio = f"{float(host.lstrip('~')) / min(ms):.1f}" if host else "-"
            lines.append(f"{n:>6} {comb(n, 4):>14} {host or '-':>12} {min(ms):>10.3f} {max(ms):>10.3f} {ratio:>12} "
                         f"{comb(n, 4) / min(ms) / 1e6:>9.1f} {launches:>9} {min(ms) / launches:>10.3f} {min(owner_ms):>10.3f}  {same}  {owner_same}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
