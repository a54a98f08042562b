// Host side of the taxon axis (pf_forward_taxa, pf_forward_leave_one_out): the table check and the pair-index rules.
// Plain C++, no HIP: tests/native/pf_taxa_shim.cpp drives it under AddressSanitizer / UBSan; pf_taxa.hip.h compiles
// the index rules for the device too (PF_TAXA_HD).
//
// Pair order (phyloformer_amd/taxa.py::pair_index is the host twin): the reference's, the row-major upper triangle -
// pair (i, j), i < j, of N rows has index  i (2N - i - 1) / 2 + (j - i - 1).
// Leave-one-out: set t is the alignment without row t, the remaining rows in order; row r != t sits at r - (r > t)
// there, so pair (i, j) - neither of them t - has the index of (i - (i > t), j - (j > t)) among N - 1 rows.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_TAXA_HD __host__ __device__
#else
#define PF_TAXA_HD
#endif

namespace pftaxa {

// index of the first entry of table[n] outside [0, N), or -1: one branch-free pass the compiler vectorises, the
// offender is looked for only if there is one
inline int64_t first_bad_taxon(const int32_t* table, size_t n, int N) {
    unsigned bad = 0;
    for (size_t i = 0; i < n; ++i) bad |= (unsigned)((uint32_t)table[i] >= (uint32_t)N);
    if (bad)
        for (size_t i = 0; i < n; ++i)
            if ((uint32_t)table[i] >= (uint32_t)N) return (int64_t)i;
    return -1;
}

// index of the first pair of row i (for i = N - 1: the number of pairs)
PF_TAXA_HD inline int64_t pair_row_start(int i, int N) { return (int64_t)i * (2 * (int64_t)N - i - 1) / 2; }

// index of pair (i, j), 0 <= i < j < N, or -1
PF_TAXA_HD inline int64_t pair_index(int i, int j, int N) {
    if (i < 0 || j <= i || j >= N) return -1;
    return pair_row_start(i, N) + (j - i - 1);
}

// the pair (i, j) of index q among N rows; false (i = j = -1) for q outside [0, N (N - 1) / 2)
PF_TAXA_HD inline bool pair_of(int64_t q, int N, int* i, int* j) {
    *i = *j = -1;
    if (N < 2 || q < 0 || q >= pair_row_start(N - 1, N)) return false;
    // row = the largest r with pair_row_start(r) <= q: the root of r^2 - (2N - 1) r + 2q = 0, then an exact correction
    const double b = 2.0 * (double)N - 1.0;
    const double disc = b * b - 8.0 * (double)q;                // >= 9 exactly; rounding may take it below 0 for huge N
    int r = (int)((b - sqrt(disc > 0.0 ? disc : 0.0)) * 0.5);
    if (r < 0) r = 0;
    if (r > N - 2) r = N - 2;
    while (r > 0 && pair_row_start(r, N) > q) --r;
    while (r < N - 2 && pair_row_start(r + 1, N) <= q) ++r;
    *i = r;
    *j = r + 1 + (int)(q - pair_row_start(r, N));
    return true;
}

// index of pair (i, j) of the N rows in the leave-one-out set t (N - 1 rows), or -1 (t is i or j, or a bad argument)
PF_TAXA_HD inline int64_t loo_pair_index(int i, int j, int t, int N) {
    if (t < 0 || t >= N || i == t || j == t || i < 0 || j <= i || j >= N) return -1;
    return pair_index(i - (i > t ? 1 : 0), j - (j > t ? 1 : 0), N - 1);
}

}  // namespace pftaxa
