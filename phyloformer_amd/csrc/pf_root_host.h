// Tree rooting (pf_tree_root, pf_tree_root_device, pf_tree_root_host): the minimal-ancestor-deviation score
// and root position of every branch of a join table (Tria, Landan & Dagan 2017) and the midpoint of its longest path.  Plain C++,
// no HIP: tests/native/pf_root_main.cpp runs the serial twin under AddressSanitizer / UBSan, pf_root.hip.h compiles the bodies
// for the device too (PF_TAXA_HD).  phyloformer_amd/root.py is the statement: every float64 operation here happens with the same
// operands and in the same order as there, nothing contracts (the bodies switch contraction off; a g++ build passes
// -ffp-contract=off), so the arrays are bit-identical.
//
// Nodes, kids, cnt, lo and ord are pf_ols_host.h's; parent / L [2N - 2] are the parent and the clamped length above every node.
// Columns are in tree leaf order: q = lo[x] is the place of leaf x, D [2N - 2][N] holds at [v][q] the path from node v to the leaf
// at q, Wt [N][N] holds at [c][q] the weight W[q][c] of the leaves at q and c - transposed, so that consecutive q are neighbours
// in memory for a fixed c.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pf_fit_host.h"
#include "pf_ols_host.h"
#include "pf_spans.h"
#include "pf_taxa_host.h"

namespace pfroot {

using pffit::LANES;
using pffit::MAX_N;
using pffit::MIN_N;
using pffit::NO_TABLE;
using pffit::NONFINITE;
using pffit::OK;
using pffit::nodes_of;
using pffit::table_len;

constexpr int MID = 5;      // mid: k, lam_mid, b, c, D[c][b]

// what the three entry points refuse about (B, M, N): 0, or which (1: N below, 2: N above, 3: B, 4: M)
inline int refused(int B, int M, int N) { return pfols::refused(B, M, N); }

PF_TAXA_HD inline double clamp_length(double x) { return x > 0.0 ? x : 0.0; }
PF_TAXA_HD inline bool below(int lo_v, int n_v, int q) { return q >= lo_v && q < lo_v + n_v; }

// parent and L of the node behind entry k of the table
PF_TAXA_HD inline void node_of_entry(const int32_t* kids, const double* lengths, int N, int k, int32_t* parent, double* L) {
    const int v = kids[k];
    parent[v] = k < 2 * (N - 3) ? N + (k >> 1) : 2 * N - 3;
    L[v] = clamp_length(lengths[k]);
}

// column q of D (leaf x = ord[q]): upward from the leaf, then every node x is not below, in descending order
PF_TAXA_HD inline void column(const int32_t* parent, const double* L, const int32_t* cnt, const int32_t* lo, int N, int q, int x, double* D) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t n = (size_t)N;
    const int root = 2 * N - 3;
    D[(size_t)x * n + q] = 0.0;
    for (int v = x; v != root;) {
        const int p = parent[v];
        D[(size_t)p * n + q] = D[(size_t)v * n + q] + L[v];
        v = p;
    }
    for (int v = root - 1; v >= 0; --v)
        if (!below(lo[v], cnt[v], q)) D[(size_t)v * n + q] = D[(size_t)parent[v] * n + q] + L[v];
}

PF_TAXA_HD inline double weight(double d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(d > 0.0)) return 0.0;
    const double dd = d * d;
    return 1.0 / dd;
}

// One of the 64 strided accumulators of a branch's position sums.
struct Part {
    double s1, s0;
};

// lane `lane` of the position pass of node v: q = lo_v + lane, + 64, ... ascending, each with its sums over the c outside the range
PF_TAXA_HD inline Part position_lane(const double* D, const double* Wt, int N, int v, int lo_v, int n_v, int lane) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t n = (size_t)N;
    const double* dv = D + (size_t)v * n;
    Part p{0.0, 0.0};
    for (int j = lane; j < n_v; j += LANES) {
        const int q = lo_v + j;
        const double dq = dv[q];
        double r1 = 0.0, r0 = 0.0;
        for (int c = 0; c < N; ++c) {
            if (c == lo_v) { c += n_v - 1; continue; }
            const double w = Wt[(size_t)c * n + q];
            const double diff = dq - dv[c];
            const double wd = w * diff;
            r1 = r1 + wd;
            r0 = r0 + w;
        }
        p.s1 = p.s1 + r1;
        p.s0 = p.s0 + r0;
    }
    return p;
}

PF_TAXA_HD inline void part_merge(Part& p, const Part& o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    p.s1 = p.s1 + o.s1;
    p.s0 = p.s0 + o.s0;
}

// the root's distance above the node from the combined sums
PF_TAXA_HD inline double position(const Part& s, double Lv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (s.s0 == 0.0) return 0.0;
    const double den = 2.0 * s.s0;
    double x = -s.s1 / den;
    x = x > 0.0 ? x : 0.0;
    return x < Lv ? x : Lv;
}

// the root-to-tip distance of the leaf at a place in the range (inside) or outside it
PF_TAXA_HD inline double tip(double dvq, double lam, bool inside) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return inside ? dvq + lam : dvq - lam;
}

// one term of the score
PF_TAXA_HD inline double term(double w, double tq, double tc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double diff = tq - tc;
    const double dd = diff * diff;
    return w * dd;
}

// lane `lane` of the score pass of node v with its root at lam: q = lane, lane + 64, ... ascending over all places
PF_TAXA_HD inline double score_lane(const double* D, const double* Wt, int N, int v, int lo_v, int n_v, double lam, int lane) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t n = (size_t)N;
    const double* dv = D + (size_t)v * n;
    double acc = 0.0;
    for (int q = lane; q < N; q += LANES) {
        const double tq = tip(dv[q], lam, below(lo_v, n_v, q));
        double r = 0.0;
        for (int c = 0; c < N; ++c) r = r + term(Wt[(size_t)c * n + q], tq, tip(dv[c], lam, below(lo_v, n_v, c)));
        acc = acc + r;
    }
    return acc;
}

// The farthest pair so far: D[c][b] of leaves b < c, the first in pair order among equals.
struct Far {
    double d;
    int32_t b, c;
};
PF_TAXA_HD inline Far far_none() { return Far{-1.0, 0, 0}; }
PF_TAXA_HD inline void far_take(Far& f, const Far& o) {
    if (o.d > f.d || (o.d == f.d && (o.b < f.b || (o.b == f.b && o.c < f.c)))) f = o;
}

// does the branch of entry k hold the midpoint of the path of b and c?  lam: its distance above the branch's lower node
PF_TAXA_HD inline bool mid_entry(const double* D, const int32_t* kids, const int32_t* parent, const int32_t* cnt, const int32_t* lo, int N,
                                 int k, int b, int c, double half, double* lam) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t n = (size_t)N;
    const int v = kids[k], p = parent[v], qb = lo[b];
    const bool has_b = below(lo[v], cnt[v], qb), has_c = below(lo[v], cnt[v], lo[c]);
    if (has_b == has_c) return false;
    const double at_v = D[(size_t)v * n + qb], at_p = D[(size_t)p * n + qb];
    if (has_b) {
        if (!(at_v <= half && half <= at_p)) return false;
        *lam = half - at_v;
    } else {
        if (!(at_p <= half && half <= at_v)) return false;
        *lam = at_v - half;
    }
    return true;
}

// One tree, serially: ssq [T], pos [T], mid [5] (zeroed here), the status.
inline void run_serial(const int32_t* slots, const double* lengths, int N, double* ssq, double* pos, double* mid, uint8_t* status) {
    const int T = table_len(N), nodes = nodes_of(N);
    const size_t n = (size_t)N;
    for (int k = 0; k < T; ++k) ssq[k] = pos[k] = 0.0;
    for (int k = 0; k < MID; ++k) mid[k] = 0.0;
    std::vector<int32_t> node(n), kids((size_t)T), cnt((size_t)nodes, 1), lo((size_t)nodes), ord(n), parent((size_t)nodes);
    *status = pfols::replay_kids(slots, N, node.data(), kids.data());
    if (*status != OK) return;
    bool bad = false;
    for (int k = 0; k < T; ++k) bad |= pffit::nonfinite(lengths[k]);
    if (bad) { *status = NONFINITE; return; }
    pfols::count_leaves(kids.data(), N, cnt.data());
    pfols::leaf_offsets(kids.data(), N, cnt.data(), lo.data());
    for (int x = 0; x < N; ++x) ord[(size_t)lo[(size_t)x]] = x;
    std::vector<double> L((size_t)nodes), D((size_t)nodes * n), Wt(n * n);
    for (int k = 0; k < T; ++k) node_of_entry(kids.data(), lengths, N, k, parent.data(), L.data());
    parent[(size_t)nodes - 1] = nodes - 1; L[(size_t)nodes - 1] = 0.0;
    for (int q = 0; q < N; ++q) column(parent.data(), L.data(), cnt.data(), lo.data(), N, q, ord[(size_t)q], D.data());
    for (int c = 0; c < N; ++c)
        for (int q = 0; q < N; ++q) Wt[(size_t)c * n + q] = weight(D[(size_t)ord[(size_t)q] * n + c]);
    Part parts[LANES];
    double acc[LANES];
    for (int k = 0; k < T; ++k) {
        const int v = kids[(size_t)k], lo_v = lo[(size_t)v], n_v = cnt[(size_t)v];
        for (int l = 0; l < LANES; ++l) parts[l] = position_lane(D.data(), Wt.data(), N, v, lo_v, n_v, l);
        for (int s = LANES / 2; s > 0; s >>= 1)
            for (int l = 0; l < s; ++l) part_merge(parts[l], parts[l + s]);
        pos[k] = position(parts[0], L[(size_t)v]);
        for (int l = 0; l < LANES; ++l) acc[l] = score_lane(D.data(), Wt.data(), N, v, lo_v, n_v, pos[k], l);
        for (int s = LANES / 2; s > 0; s >>= 1)
            for (int l = 0; l < s; ++l) acc[l] = acc[l] + acc[l + s];
        ssq[k] = 0.5 * acc[0];
    }
    Far far = far_none();
    for (int c = 1; c < N; ++c)
        for (int b = 0; b < c; ++b) far_take(far, Far{D[(size_t)c * n + (size_t)lo[(size_t)b]], b, c});
    const double half = 0.5 * far.d;
    for (int k = 0; k < T; ++k) {
        double lam = 0.0;
        if (!mid_entry(D.data(), kids.data(), parent.data(), cnt.data(), lo.data(), N, k, far.b, far.c, half, &lam)) continue;
        mid[0] = (double)k; mid[1] = lam; mid[2] = (double)far.b; mid[3] = (double)far.c; mid[4] = far.d;
        break;
    }
}

// The arrays of a call as the caller or the staging of a host call holds them: B sources of M trees each.
struct Tables {
    const int32_t* slots; const double* lengths;
    double* ssq; double* pos; double* mid; uint8_t* status;
};
template <class V>
inline void staging_arrays(V& v, Tables& s, const Tables& u, size_t B, size_t M, int N) {
    const size_t T = (size_t)(N >= 3 ? table_len(N) : 0);
    v.in(s.lengths, u.lengths, B * M * T);
    v.out(s.ssq, u.ssq, B * M * T);
    v.out(s.pos, u.pos, B * M * T);
    v.out(s.mid, u.mid, B * M * MID);
    v.in(s.slots, u.slots, B * M * T);
    v.out(s.status, u.status, B * M);
}

}  // namespace pfroot
