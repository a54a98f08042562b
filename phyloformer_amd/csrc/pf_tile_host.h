// Host side of tiled inference (pf_forward_tiled, pf_tile_combine_device, pf_tile_groups, pf_tile_bound): the covering
// plan, and the body of k_tile_combine (combine_row) as a function of (row, source, thread).  Plain C++, no HIP:
// tests/native/pf_tile_main.cpp runs both on the CPU under AddressSanitizer / UBSan; pf_tile.hip.h compiles them for the
// device too (PF_TAXA_HD).  phyloformer_amd/tile.py::plan and ::combine are the Python twins.
//
// N sequences, a context of M rows, 2 <= M, N > M:
//   G = ceil(N / floor(M / 2)) groups (N > M implies G >= 3); group g is the contiguous rows
//   [floor(g N / G), floor((g + 1) N / G)): sizes differ by at most one, none is empty, and two of them fit M.
//   Set (g, h), g < h, in lexicographic order - its number is pair_index(g, h, G) - is the rows of group g followed by
//   the rows of group h, ascending: m = n_g + n_h <= M rows, m (m - 1) / 2 distances in the reference's pair order
//   (pf_taxa_host.h).  S = G (G - 1) / 2 sets of at most three distinct sizes; T = the sum of their distance counts.
//   A cross-group pair lies in exactly one set, a within-group pair of group g in the G - 1 sets that contain g.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pf_taxa_host.h"

namespace pftile {

// G, or -1 for M < 2 or N <= M
inline int64_t groups(int64_t N, int64_t M) {
    if (M < 2 || N <= M) return -1;
    const int64_t half = M / 2;
    return (N + half - 1) / half;
}

// first row of group g (g = G: N)
PF_TAXA_HD inline int64_t bound(int64_t N, int64_t G, int64_t g) { return g * N / G; }

// the group of row i: the largest g with floor(g N / G) <= i
PF_TAXA_HD inline int64_t group_of(int64_t N, int64_t G, int64_t i) { return ((i + 1) * G - 1) / N; }

// number of set (g, h), 0 <= g < h < G, in lexicographic order
PF_TAXA_HD inline int64_t set_index(int64_t g, int64_t h, int64_t G) { return g * (2 * G - g - 1) / 2 + (h - g - 1); }

// The plan of (N, M) as the tables the driver and k_tile_combine read.
struct Plan {
    int N = 0, M = 0, G = 0;
    int64_t S = 0, T = 0;              // sets; distances of all sets of one source
    std::vector<int32_t> bounds;       // [G + 1]: first row of every group, then N
    std::vector<int64_t> offset;       // [S + 1]: first distance of every set in [T], then T
    int n_class = 0;                   // distinct set sizes, ascending
    int class_m[3] = {0, 0, 0};
    int64_t class_sets[3] = {0, 0, 0};

    int rows(int64_t g) const { return bounds[(size_t)g + 1] - bounds[(size_t)g]; }
    int class_of(int m) const {
        for (int c = 0; c < n_class; ++c)
            if (class_m[c] == m) return c;
        return -1;
    }

    // false for M < 2, N <= M or N >= 2^31 (throws std::bad_alloc like any vector)
    bool build(int64_t n, int64_t m) {
        const int64_t g = groups(n, m);
        if (g < 0 || n > INT32_MAX) return false;
        N = (int)n; M = (int)m; G = (int)g;
        S = g * (g - 1) / 2;
        bounds.resize((size_t)G + 1);
        for (int64_t k = 0; k <= g; ++k) bounds[(size_t)k] = (int32_t)bound(n, g, k);
        offset.resize((size_t)S + 1);
        n_class = 0;
        for (int c = 0; c < 3; ++c) class_m[c] = 0, class_sets[c] = 0;
        const int lo = 2 * (int)(n / g);               // group sizes are floor(N / G) or one more
        int64_t at = 0, k = 0;
        int64_t count[3] = {0, 0, 0};
        for (int a = 0; a < G; ++a)
            for (int b = a + 1; b < G; ++b, ++k) {
                const int sz = rows(a) + rows(b);
                offset[(size_t)k] = at;
                at += (int64_t)sz * (sz - 1) / 2;
                ++count[sz - lo];
            }
        offset[(size_t)S] = T = at;
        for (int d = 0; d < 3; ++d)
            if (count[d]) class_m[n_class] = lo + d, class_sets[n_class] = count[d], ++n_class;
        return true;
    }
};

// the plan's two tables on the device
struct Tables { int64_t* offset = nullptr; int32_t* bounds = nullptr; };
template <class V>
inline void table_arrays(V& v, Tables& t, const Plan& p) {
    v(t.offset, p.offset.size());
    v(t.bounds, p.bounds.size());
}

// What k_tile_combine reads and writes (pf_tile.hip.h has the definitions of out and spread).
struct CombineArgs {
    const float* sets;       // [B][T]
    const int32_t* bounds;   // [G + 1]
    const int64_t* offset;   // [S + 1]
    float* out;              // [B][P_N]
    float* spread;           // [B][P_N]
    int N, G;
    int64_t T, PN;
};

// Thread `tid` of `threads` on output row i < N - 1 of source b: the pairs (i, j), j = i + 1 + tid, + threads, ...
// No contraction: the twin rounds the product and the sum of (d - mean)^2 separately.
PF_TAXA_HD inline void combine_row(const CombineArgs& a, int i, size_t b, int tid, int threads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int N = a.N, G = a.G;
    const int g = (int)group_of(N, G, i);
    const int bg = a.bounds[g], ng = a.bounds[g + 1] - bg, il = i - bg;
    const float* sets = a.sets + b * (size_t)a.T;
    const int64_t row = (int64_t)b * a.PN + pftaxa::pair_row_start(i, N) - i - 1;      // + j: pair (i, j)
    float* out = a.out + row;
    float* spread = a.spread + row;

    // within the group: j in (i, bg + ng), G - 1 values each, in ascending order of the partner group p
    for (int j = i + 1 + tid; j < bg + ng; j += threads) {
        const int jl = j - bg;
        double sum = 0.0;
        for (int p = 0; p < G; ++p) {
            if (p == g) continue;
            const int np = a.bounds[p + 1] - a.bounds[p];
            const int64_t at = p < g ? a.offset[set_index(p, g, G)] + pftaxa::pair_index(np + il, np + jl, np + ng)
                                     : a.offset[set_index(g, p, G)] + pftaxa::pair_index(il, jl, ng + np);
            sum += (double)sets[at];
        }
        const double mean = sum / (double)(G - 1);
        double ss = 0.0;
        for (int p = 0; p < G; ++p) {
            if (p == g) continue;
            const int np = a.bounds[p + 1] - a.bounds[p];
            const int64_t at = p < g ? a.offset[set_index(p, g, G)] + pftaxa::pair_index(np + il, np + jl, np + ng)
                                     : a.offset[set_index(g, p, G)] + pftaxa::pair_index(il, jl, ng + np);
            const double d = (double)sets[at] - mean;
            ss += d * d;
        }
        out[j] = (float)mean;
        spread[j] = (float)sqrt(ss / (double)(G - 2));
    }

    // across groups: j >= bg + ng, one value each; a thread's j only grows, and so does its partner group h
    int h = g + 1;
    for (int j = bg + ng + tid; j < N; j += threads) {
        while (a.bounds[h + 1] <= j) ++h;                              // (bounds[G] = N > j ends it)
        const int bh = a.bounds[h], nh = a.bounds[h + 1] - bh;
        out[j] = sets[a.offset[set_index(g, h, G)] + pftaxa::pair_index(il, ng + (j - bh), ng + nh)];
        spread[j] = 0.0f;
    }
}

}  // namespace pftile
