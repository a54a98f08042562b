#!/usr/bin/env python3
"""Fuzz driver of the site-weight host code (csrc/pf_weights_host.h) under AddressSanitizer + UBSan (run by
tests/test_native_sanitizers_weights.py in a child process with libasan preloaded; any sanitizer report aborts the
process, any mismatch raises).

  * padded_sites on the whole int32 range (the rounding up must not overflow);
  * boot_counts and compress_sites on exact-size buffers (an overrun lands in a red zone) against
    phyloformer_amd/weights_sites.py, shapes from 1 x 1 up, alphabets from one letter (all columns identical) to no repeats;
  * first_bad_weight on exact-size arrays: valid weights, one offender anywhere (negative, -0.0 is valid, NaN, +-inf),
    empty arrays; weight_sum against numpy's sequential float32 sum.
"""
import ctypes as C
import os
import sys

import numpy as np
from hypothesis import HealthCheck, given, settings, strategies as st

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from phyloformer_amd import weights_sites as ws  # noqa: E402

LIB = C.CDLL(sys.argv[1])
EXAMPLES = int(sys.argv[2]) if len(sys.argv) > 2 else 300
CFG = dict(max_examples=EXAMPLES, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
I32 = 2 ** 31 - 1
LIB.t_padded_sites.argtypes = [C.c_int, C.c_int]
LIB.t_boot_counts.argtypes = [C.c_int, C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p]
LIB.t_compress_slots.restype = C.c_longlong
LIB.t_compress_slots.argtypes = [C.c_int]
LIB.t_compress_sites.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
LIB.t_first_bad_weight.restype = C.c_longlong
LIB.t_first_bad_weight.argtypes = [C.c_void_p, C.c_longlong]
LIB.t_weight_sum.restype = C.c_float
LIB.t_weight_sum.argtypes = [C.c_void_p, C.c_int]
i32 = st.integers(-I32 - 1, I32)


@settings(**CFG)
@given(i32, i32)
def padding(K, L):
    got = LIB.t_padded_sites(K, L)
    if K < 1 or K > L:
        assert got == -1
    else:
        assert got == min(L, 32 * ((K + 31) // 32)) and K <= got <= L


@settings(**CFG)
@given(st.integers(1, 400), st.integers(0, 2 ** 64 - 1), st.integers(0, I32))
def boot(L, seed, r):
    sites = np.empty(L, np.int32)
    counts = np.empty(L, np.int32)                     # exact size: nothing past them may be touched
    K = LIB.t_boot_counts(L, seed, r, sites.ctypes.data, counts.ctypes.data)
    want = ws.boot_counts(L, r + 1, seed, r)
    assert K == len(want[0]) and np.array_equal(sites[:K], want[0]) and np.array_equal(counts[:K], want[1])
    assert LIB.t_boot_counts(0, seed, r, None, None) == -1 and LIB.t_boot_counts(L, seed, -1, None, None) == -1


@settings(**CFG)
@given(st.integers(1, 6), st.integers(1, 200), st.integers(1, 22), st.integers(0, 2 ** 32 - 1))
def compress(N, L, letters, seed):
    idx = np.random.default_rng(seed).integers(0, letters, (N, L)).astype(np.uint8)
    first = np.empty(L, np.int32)
    count = np.empty(L, np.int32)
    slot = np.empty(LIB.t_compress_slots(L), np.int32)
    assert len(slot) >= 2 * L and len(slot) & (len(slot) - 1) == 0
    K = LIB.t_compress_sites(idx.ctypes.data, N, L, first.ctypes.data, count.ctypes.data, slot.ctypes.data)
    want = ws.compress_sites(idx)
    assert K == len(want[0]) and np.array_equal(first[:K], want[0]) and np.array_equal(count[:K], want[1])


@settings(**CFG)
@given(st.integers(0, 300), st.data())
def weights(n, data):
    rng = np.random.default_rng(data.draw(st.integers(0, 2 ** 32 - 1)))
    w = (rng.random(n) * 4).astype(np.float32)
    if n:
        w[rng.integers(0, n)] = 0.0
        w[rng.integers(0, n)] = -0.0
    assert LIB.t_first_bad_weight(w.ctypes.data if n else None, n) == -1
    if n:
        acc = np.float32(0)
        for v in w:
            acc = np.float32(acc + v)
        assert LIB.t_weight_sum(w.ctypes.data, n) == acc
        at = sorted(data.draw(st.lists(st.integers(0, n - 1), min_size=1, max_size=3)))
        for k in at:
            w[k] = data.draw(st.sampled_from([-1.0, -1e-30, float("nan"), float("inf"), float("-inf")]))
        assert LIB.t_first_bad_weight(w.ctypes.data, n) == at[0]


if __name__ == "__main__":
    padding()
    boot()
    compress()
    weights()
    assert LIB.t_padded_sites(I32, I32) == I32 and LIB.t_padded_sites(I32 - 40, I32) == I32 - 31
    print("fuzz_weights: clean")
