// Host side of the site maps (pf_window_count, pf_window_start, the table check of pf_forward_sites).  Plain C++, no
// HIP: tests/native/pf_sites_shim.cpp drives it under AddressSanitizer / UBSan.
//
// The window rule (phyloformer_amd/windows.py::window_starts is its host twin): windows of W sites start at
// 0, step, 2 step, ... while start + W <= L; if the last of them ends before L, one more window is anchored at L - W,
// so that every site is covered.  W == L gives one window.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pfsites {

// number of windows, or -1 for W < 1, W > L, step < 1 (or a count that does not fit an int)
inline int window_count(int L, int W, int step) {
    if (W < 1 || W > L || step < 1) return -1;
    int64_t n = (int64_t)(L - W) / step + 1;
    if ((n - 1) * (int64_t)step + W < L) ++n;
    return n > INT32_MAX ? -1 : (int)n;
}

// first site (0-based) of window s, or -1 for a bad rule or s outside [0, window_count)
inline int window_start(int L, int W, int step, int s) {
    const int n = window_count(L, W, step);
    if (n < 0 || s < 0 || s >= n) return -1;
    const int64_t st = (int64_t)s * step;
    return st + W <= L ? (int)st : L - W;
}

// index of the first entry of sites[n] outside [0, L), or -1: one branch-free pass the compiler vectorises, the
// offender is looked for only if there is one
inline int64_t first_bad_site(const int32_t* sites, size_t n, int L) {
    unsigned bad = 0;
    for (size_t i = 0; i < n; ++i) bad |= (unsigned)((uint32_t)sites[i] >= (uint32_t)L);
    if (bad)
        for (size_t i = 0; i < n; ++i)
            if ((uint32_t)sites[i] >= (uint32_t)L) return (int64_t)i;
    return -1;
}

}  // namespace pfsites
