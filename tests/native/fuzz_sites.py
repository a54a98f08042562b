#!/usr/bin/env python3
"""Fuzz driver of the site-map host code (csrc/pf_sites_host.h) under AddressSanitizer + UBSan (run by
tests/test_native_sanitizers_sites.py in a child process with libasan preloaded; any sanitizer report aborts the
process, any mismatch raises).

  * window_count / window_start against phyloformer_amd/windows.py::window_starts on hypothesis-generated (L, W, step),
    the whole int32 range included (signed overflow of s * step or (n - 1) * step + W would be a UBSan report), bad
    rules and window indices one outside the range;
  * first_bad_site on exact-size tables (an overrun lands in a red zone): valid tables, one offender anywhere,
    INT32_MIN / INT32_MAX entries, empty tables, L from 1 to INT32_MAX.
"""
import ctypes as C
import os
import sys

import numpy as np
from hypothesis import HealthCheck, given, settings, strategies as st

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from phyloformer_amd.windows import window_starts  # noqa: E402

LIB = C.CDLL(sys.argv[1])
EXAMPLES = int(sys.argv[2]) if len(sys.argv) > 2 else 300
CFG = dict(max_examples=EXAMPLES, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
I32 = 2 ** 31 - 1
LIB.t_window_count.argtypes = [C.c_int] * 3
LIB.t_window_start.argtypes = [C.c_int] * 4
LIB.t_first_bad_site.restype = C.c_longlong
LIB.t_first_bad_site.argtypes = [C.c_void_p, C.c_longlong, C.c_int]
i32 = st.integers(-I32 - 1, I32)


def closed_form(L, W, step):
    """The rule without materialising the starts (L may be 2^31 - 1)."""
    n = (L - W) // step + 1
    return n + 1 if (n - 1) * step + W < L else n


@settings(**CFG)
@given(st.integers(1, 3000), st.data())
def small_rules(L, data):
    W = data.draw(st.integers(1, L))
    step = data.draw(st.integers(1, 2 * L + 1))
    want = window_starts(L, W, step)
    assert LIB.t_window_count(L, W, step) == len(want) == closed_form(L, W, step)
    assert [LIB.t_window_start(L, W, step, s) for s in range(len(want))] == want
    assert LIB.t_window_start(L, W, step, len(want)) == -1 and LIB.t_window_start(L, W, step, -1) == -1


@settings(**CFG)
@given(i32, i32, i32, i32)
def any_rule(L, W, step, s):
    n = LIB.t_window_count(L, W, step)
    if W < 1 or W > L or step < 1:
        assert n == -1 and LIB.t_window_start(L, W, step, s) == -1
        return
    assert n == closed_form(L, W, step) >= 1
    for k in {s, 0, n - 1, n, -1, n // 2}:
        got = LIB.t_window_start(L, W, step, k)
        if 0 <= k < n:
            assert got == (k * step if k * step + W <= L else L - W) and 0 <= got <= L - W
        else:
            assert got == -1


@settings(**CFG)
@given(st.integers(1, I32), st.integers(0, 300), st.data())
def tables(L, n, data):
    rng = np.random.default_rng(data.draw(st.integers(0, 2 ** 32 - 1)))
    tab = rng.integers(0, L, size=n, dtype=np.int64).astype(np.int32)       # exact size: nothing past it may be read
    assert LIB.t_first_bad_site(tab.ctypes.data if n else None, n, L) == -1
    if n:
        at = sorted(data.draw(st.lists(st.integers(0, n - 1), min_size=1, max_size=3)))
        for k in at:
            tab[k] = data.draw(st.sampled_from([-1, -I32 - 1, L if L < I32 else -2, I32 if L < I32 else -3]))
        assert LIB.t_first_bad_site(tab.ctypes.data, n, L) == at[0]


if __name__ == "__main__":
    small_rules()
    any_rule()
    tables()
    assert LIB.t_window_count(I32, 1, 1) == I32 and LIB.t_window_start(I32, 1, 1, I32 - 1) == I32 - 1
    assert LIB.t_window_count(I32, I32, I32) == 1 and LIB.t_window_count(I32, 1, I32) == 2
    assert LIB.t_window_start(I32, 1, I32, 1) == I32 - 1
    print("fuzz_sites: clean")
