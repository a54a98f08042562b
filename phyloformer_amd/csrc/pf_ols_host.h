// Least-squares branch lengths (pf_tree_ols, pf_tree_ols_device, pf_tree_ols_host): the lengths that
// reproduce the distances best on a FIXED join table, by the closed form of Rzhetsky & Nei 1993 (FastME's -w OLS).  Plain C++,
// no HIP: tests/native/pf_ols_main.cpp runs the serial twin under AddressSanitizer / UBSan, pf_ols.hip.h compiles the bodies
// for the device too (PF_TAXA_HD).  phyloformer_amd/ols.py is the statement: every float64 operation here happens with the same
// operands and in the same order as there, nothing contracts (the bodies switch contraction off; a g++ build passes
// -ffp-contract=off), so the arrays are bit-identical.
//
// Nodes are pf_fit_host.h's.  kids [T] names the node behind every entry of the table: the children of node N + t at 2t and
// 2t + 1, those of the last node R = 2N - 3 at 2 (N - 3) + k; the branch above kids[k] is ols[k].  cnt [2N - 2] counts a node's
// leaves; ord [N] lists the leaves so that those of node v are ord[lo[v] .. lo[v] + cnt[v]).  W [2N - 2][N]: row v < R holds, per
// leaf x, the sum of x's distances to the leaves of v; row R holds r.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pf_fit_host.h"
#include "pf_spans.h"
#include "pf_taxa_host.h"

namespace pfols {

using pffit::LANES;
using pffit::MAX_N;
using pffit::MIN_N;
using pffit::NO_TABLE;
using pffit::NONFINITE;
using pffit::OK;
using pffit::nodes_of;
using pffit::table_len;

// what the three entry points refuse about (B, M, N): 0, or which (1: N below, 2: N above, 3: B, 4: M)
inline int refused(int B, int M, int N) {
    if (N < MIN_N) return 1;
    if (N > MAX_N) return 2;
    if (B < 1) return 3;
    if (M < 1) return 4;
    return 0;
}

// The table replayed by ONE thread with pf_fit_host.h::replay's checks: kids [T]; `node` [N] is scratch (the node in every
// slot, -1 once the slot has left).  `kids` may be `slots` itself.  NO_TABLE or OK; nothing is read or written out of bounds
// for any table.
PF_TAXA_HD inline uint8_t replay_kids(const int32_t* slots, int N, int32_t* node, int32_t* kids) {
    for (int s = 0; s < N; ++s) node[s] = s;
    const int J = N - 3;
    for (int t = 0; t < J; ++t) {
        const int32_t a = slots[2 * t], b = slots[2 * t + 1];
        if (a < 0 || a >= N || b < 0 || b >= N || a == b || node[a] < 0 || node[b] < 0) return NO_TABLE;
        kids[2 * t] = node[a]; kids[2 * t + 1] = node[b];
        node[a] = N + t; node[b] = -1;
    }
    for (int k = 0; k < 3; ++k) {
        const int32_t s = slots[2 * J + k];
        if (s < 0 || s >= N || node[s] < 0) return NO_TABLE;      // (a repeated slot has left by its second use)
        kids[2 * J + k] = node[s];
        node[s] = -1;
    }
    return OK;
}

// cnt [2N - 2] of the join nodes and the last node, in ascending node order; the leaves' entries are 1 already
PF_TAXA_HD inline void count_leaves(const int32_t* kids, int N, int32_t* cnt) {
    for (int t = 0; t < N - 3; ++t) cnt[N + t] = cnt[kids[2 * t]] + cnt[kids[2 * t + 1]];
    cnt[2 * N - 3] = N;
}

// lo [2N - 2] in descending node order.  `lo` may be `cnt` itself: a node's count is read for the last time when its parent
// is visited, its offset is written then and read when the node itself is visited, later.
PF_TAXA_HD inline void leaf_offsets(const int32_t* kids, int N, const int32_t* cnt, int32_t* lo) {
    const int J = N - 3;
    const int32_t c0 = kids[2 * J], c1 = kids[2 * J + 1], c2 = kids[2 * J + 2];
    const int32_t n0 = cnt[c0], n1 = cnt[c1];
    lo[2 * N - 3] = 0;
    lo[c0] = 0; lo[c1] = n0; lo[c2] = n0 + n1;
    for (int t = J - 1; t >= 0; --t) {
        const int32_t a = kids[2 * t], b = kids[2 * t + 1];
        const int32_t at = lo[N + t], na = cnt[a];
        lo[a] = at; lo[b] = at + na;
    }
}

// The branch of entry k of the table: the node v below it, its sibling side C, and the far side D as the rows of W that make
// f_D[x] = W[frow][x] - W[grow][x] (grow < 0: W[frow][x] alone) with its leaf count nd.
struct Branch {
    int32_t v, c, frow, grow, nc, nd;
};
PF_TAXA_HD inline Branch branch_of(const int32_t* kids, const int32_t* cnt, int N, int k) {
    const int J = N - 3, root = 2 * N - 3;
    Branch br;
    br.v = kids[k];
    if (k < 2 * J) {
        const int p = N + (k >> 1);
        br.c = kids[k ^ 1];
        br.frow = root; br.grow = p; br.nd = N - cnt[p];
    } else {
        const int i = k - 2 * J, ic = i == 0 ? 1 : 0, id = i == 2 ? 1 : 2;      // the other two in table order
        br.c = kids[2 * J + ic];
        br.frow = kids[2 * J + id]; br.grow = -1; br.nd = cnt[br.frow];
    }
    br.nc = cnt[br.c];
    return br;
}

PF_TAXA_HD inline double far_side(const double* W, int N, const Branch& br, int x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double f = W[(size_t)br.frow * (size_t)N + x];
    if (br.grow < 0) return f;
    return f - W[(size_t)br.grow * (size_t)N + x];
}

// One of the 64 strided accumulators of a branch's six group sums.
struct Part {
    double cd, ab, ac, bc, ad, bd;
};

// lane `lane` of the branch: k = lane, lane + 64, ... ascending over the leaves of C, of a and of b (a join node v only)
PF_TAXA_HD inline Part branch_lane(const double* W, int N, const int32_t* kids, const int32_t* cnt, const int32_t* lo, const int32_t* ord,
                                   const Branch& br, int lane) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    Part p{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int32_t* sub = ord + lo[br.c];
    for (int k = lane; k < br.nc; k += LANES) p.cd = p.cd + far_side(W, N, br, sub[k]);
    if (br.v < N) return p;
    const int32_t a = kids[2 * (br.v - N)], b = kids[2 * (br.v - N) + 1];
    const double* wb = W + (size_t)b * (size_t)N;
    const double* wc = W + (size_t)br.c * (size_t)N;
    sub = ord + lo[a];
    for (int k = lane, n = cnt[a]; k < n; k += LANES) {
        const int x = sub[k];
        p.ab = p.ab + wb[x];
        p.ac = p.ac + wc[x];
        p.ad = p.ad + far_side(W, N, br, x);
    }
    sub = ord + lo[b];
    for (int k = lane, n = cnt[b]; k < n; k += LANES) {
        const int x = sub[k];
        p.bc = p.bc + wc[x];
        p.bd = p.bd + far_side(W, N, br, x);
    }
    return p;
}

// lane l takes lane l + s
PF_TAXA_HD inline void part_merge(Part& p, const Part& o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    p.cd = p.cd + o.cd;
    p.ab = p.ab + o.ab;
    p.ac = p.ac + o.ac;
    p.bc = p.bc + o.bc;
    p.ad = p.ad + o.ad;
    p.bd = p.bd + o.bd;
}

PF_TAXA_HD inline double average(double s, int nx, int ny) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double pairs = (double)nx * (double)ny;
    return s / pairs;
}

// the branch's length from its combined sums
PF_TAXA_HD inline double branch_length(const double* W, int N, const int32_t* kids, const int32_t* cnt, const Branch& br, const Part& s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d_cd = average(s.cd, br.nc, br.nd);
    if (br.v < N) {
        const double up_c = W[(size_t)br.c * (size_t)N + br.v] / (double)br.nc;
        const double up_d = far_side(W, N, br, br.v) / (double)br.nd;
        const double up = up_c + up_d;
        return 0.5 * (up - d_cd);
    }
    const int na = cnt[kids[2 * (br.v - N)]], nb = cnt[kids[2 * (br.v - N) + 1]];
    const double d_ab = average(s.ab, na, nb), d_ac = average(s.ac, na, br.nc), d_bc = average(s.bc, nb, br.nc);
    const double d_ad = average(s.ad, na, br.nd), d_bd = average(s.bd, nb, br.nd);
    const double bc = (double)nb * (double)br.nc, ad = (double)na * (double)br.nd;
    const double num = bc + ad;
    const double below = (double)na + (double)nb, above = (double)br.nc + (double)br.nd;
    const double den = below * above;
    const double gamma = num / den;
    const double straight = d_ac + d_bd, crossed = d_bc + d_ad;
    const double gs = gamma * straight;
    const double rest = 1.0 - gamma;
    const double rc = rest * crossed;
    const double mixed = gs + rc;
    const double inner = d_ab + d_cd;
    return 0.5 * (mixed - inner);
}

// W[y][x] of leaves: the distance as a double, +0.0 on the diagonal
PF_TAXA_HD inline double leaf_entry(const float* pred, int N, int y, int x) {
    return x == y ? 0.0 : (double)pred[pffit::pair_at(x, y, N)];
}

// column x of W: the leaves' rows, the join nodes' in their order, r in row R
PF_TAXA_HD inline void column(const float* pred, const int32_t* kids, int N, int x, double* W) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t n = (size_t)N;
    const int J = N - 3;
    for (int y = 0; y < N; ++y) W[(size_t)y * n + x] = leaf_entry(pred, N, y, x);
    for (int t = 0; t < J; ++t) W[(size_t)(N + t) * n + x] = W[(size_t)kids[2 * t] * n + x] + W[(size_t)kids[2 * t + 1] * n + x];
    const double two = W[(size_t)kids[2 * J] * n + x] + W[(size_t)kids[2 * J + 1] * n + x];
    W[(size_t)(2 * N - 3) * n + x] = two + W[(size_t)kids[2 * J + 2] * n + x];
}

// One tree of one source, serially: ols [T] (zeroed here), the status.
inline void run_serial(const float* pred, const int32_t* slots, int N, double* ols, uint8_t* status) {
    const int64_t n = N, P = n * (n - 1) / 2;
    const int T = table_len(N), nodes = nodes_of(N);
    for (int k = 0; k < T; ++k) ols[k] = 0.0;
    std::vector<int32_t> node((size_t)N), kids((size_t)T), cnt((size_t)nodes, 1), lo((size_t)nodes), ord((size_t)N);
    *status = replay_kids(slots, N, node.data(), kids.data());
    if (*status != OK) return;
    bool bad = false;
    for (int64_t e = 0; e < P; ++e) bad |= pffit::nonfinite((double)pred[e]);
    if (bad) { *status = NONFINITE; return; }
    count_leaves(kids.data(), N, cnt.data());
    leaf_offsets(kids.data(), N, cnt.data(), lo.data());
    for (int x = 0; x < N; ++x) ord[(size_t)lo[(size_t)x]] = x;
    std::vector<double> W((size_t)nodes * (size_t)N);
    for (int x = 0; x < N; ++x) column(pred, kids.data(), N, x, W.data());
    Part lanes[LANES];
    for (int k = 0; k < T; ++k) {
        const Branch br = branch_of(kids.data(), cnt.data(), N, k);
        for (int l = 0; l < LANES; ++l) lanes[l] = branch_lane(W.data(), N, kids.data(), cnt.data(), lo.data(), ord.data(), br, l);
        for (int s = LANES / 2; s > 0; s >>= 1)
            for (int l = 0; l < s; ++l) part_merge(lanes[l], lanes[l + s]);
        ols[k] = branch_length(W.data(), N, kids.data(), cnt.data(), br, lanes[0]);
    }
}

// The arrays of a call as the caller or the staging of a host call holds them: B sources of M trees each.
struct Tables {
    const float* preds; const int32_t* slots;
    double* ols; uint8_t* status;
};
template <class V>
inline void staging_arrays(V& v, Tables& s, const Tables& u, size_t B, size_t M, int N) {
    const size_t n = (size_t)(N > 0 ? N : 0), P = n * (n > 0 ? n - 1 : 0) / 2, T = (size_t)(N >= 3 ? table_len(N) : 0);
    v.out(s.ols, u.ols, B * M * T);
    v.in(s.preds, u.preds, B * P);
    v.in(s.slots, u.slots, B * M * T);
    v.out(s.status, u.status, B * M);
}

}  // namespace pfols
