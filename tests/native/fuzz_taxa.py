#!/usr/bin/env python3
"""Fuzz driver of the taxon-axis host code (csrc/pf_taxa_host.h) under AddressSanitizer + UBSan (run by
tests/test_native_sanitizers_taxa.py in a child process with libasan preloaded; any sanitizer report aborts the
process, any mismatch raises).

  * pair_index / pair_of / loo_pair_index against phyloformer_amd/taxa.py on hypothesis-generated arguments, N up to
    32,767 (the library's pair-table range) for the round trip, the whole int32 range for the refusals (signed overflow
    of i (2N - i - 1) would be a UBSan report, an out-of-range double -> int conversion in pair_of too);
  * first_bad_taxon on exact-size tables (an overrun lands in a red zone): valid tables, offenders anywhere,
    INT32_MIN / INT32_MAX entries, empty tables, N from 1 to INT32_MAX.
"""
import ctypes as C
import os
import sys

import numpy as np
from hypothesis import HealthCheck, given, settings, strategies as st

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from phyloformer_amd import taxa as T  # noqa: E402

LIB = C.CDLL(sys.argv[1])
EXAMPLES = int(sys.argv[2]) if len(sys.argv) > 2 else 300
CFG = dict(max_examples=EXAMPLES, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
I32 = 2 ** 31 - 1
LIB.t_first_bad_taxon.restype = C.c_longlong
LIB.t_first_bad_taxon.argtypes = [C.c_void_p, C.c_longlong, C.c_int]
LIB.t_pair_index.restype = C.c_longlong
LIB.t_pair_index.argtypes = [C.c_int] * 3
LIB.t_pair_of.argtypes = [C.c_longlong, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
LIB.t_loo_pair_index.restype = C.c_longlong
LIB.t_loo_pair_index.argtypes = [C.c_int] * 4
i32 = st.integers(-I32 - 1, I32)


def pair_of(q, N):
    i, j = C.c_int(-7), C.c_int(-7)
    ok = LIB.t_pair_of(q, N, C.byref(i), C.byref(j))
    return (i.value, j.value) if ok else None


@settings(**CFG)
@given(st.integers(2, 32767), st.data())
def round_trip(N, data):
    P = N * (N - 1) // 2
    for q in {0, P - 1, data.draw(st.integers(0, P - 1)), data.draw(st.integers(0, P - 1))}:
        i, j = pair_of(q, N)
        assert 0 <= i < j < N and LIB.t_pair_index(i, j, N) == q
        if N <= 400:
            assert (i, j) == T.pair_of(q, N) and T.pair_index(i, j, N) == q
    assert pair_of(P, N) is None and pair_of(-1, N) is None
    if N >= 3:
        t = data.draw(st.integers(0, N - 1))
        i = data.draw(st.integers(0, N - 2))
        j = data.draw(st.integers(i + 1, N - 1))
        got = LIB.t_loo_pair_index(i, j, t, N)
        if t in (i, j):
            assert got == -1
        else:
            assert got == T.loo_pair_index(i, j, t, N)
            assert pair_of(got, N - 1) == (i - (i > t), j - (j > t))


@settings(**CFG)
@given(i32, i32, i32, i32, st.integers(-2 ** 63, 2 ** 63 - 1))
def any_arguments(i, j, t, N, q):
    valid = 0 <= i < j < N
    got = LIB.t_pair_index(i, j, N)
    assert got == (i * (2 * N - i - 1) // 2 + (j - i - 1) if valid else -1)
    loo = LIB.t_loo_pair_index(i, j, t, N)
    if not (valid and 0 <= t < N and t not in (i, j)):
        assert loo == -1
    else:
        assert 0 <= loo < (N - 1) * (N - 2) // 2
    res = pair_of(q, N)
    if N < 2 or not 0 <= q < N * (N - 1) // 2:
        assert res is None
    else:
        assert LIB.t_pair_index(res[0], res[1], N) == q


@settings(**CFG)
@given(st.integers(1, I32), st.integers(0, 300), st.data())
def tables(N, n, data):
    rng = np.random.default_rng(data.draw(st.integers(0, 2 ** 32 - 1)))
    tab = rng.integers(0, N, size=n, dtype=np.int64).astype(np.int32)       # exact size: nothing past it may be read
    assert LIB.t_first_bad_taxon(tab.ctypes.data if n else None, n, N) == -1
    if n:
        at = sorted(data.draw(st.lists(st.integers(0, n - 1), min_size=1, max_size=3)))
        for k in at:
            tab[k] = data.draw(st.sampled_from([-1, -I32 - 1, N if N < I32 else -2, I32 if N < I32 else -3]))
        assert LIB.t_first_bad_taxon(tab.ctypes.data, n, N) == at[0]


if __name__ == "__main__":
    round_trip()
    any_arguments()
    tables()
    assert LIB.t_pair_index(I32 - 2, I32 - 1, I32) == I32 * (I32 - 1) // 2 - 1
    assert pair_of(I32 * (I32 - 1) // 2 - 1, I32) == (I32 - 2, I32 - 1) and pair_of(0, I32) == (0, 1)
    print("fuzz_taxa: clean")
