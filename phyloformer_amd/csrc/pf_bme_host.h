// Balanced minimum-evolution NNI refinement (pf_bme_nni, pf_bme_nni_device, pf_bme_nni_host, pf_bme_newick_n; DESIGN.md
// section 21): the bodies of the kernels of pf_bme.hip.h as functions of (source, workgroup, thread), the host-side tree
// bookkeeping, and the serial driver that runs the same bodies without a device.  Plain C++, no HIP:
// tests/native/pf_bme_main.cpp runs them on the CPU thread by thread under AddressSanitizer / UBSan; pf_bme.hip.h
// compiles the bodies for the device too (PF_TAXA_HD).  phyloformer_amd/bme.py is the statement of the algorithm: tree,
// rows, balanced averages, moves, rule, lengths and the order of the output table are defined there and not repeated.
//
// Per source: d [N][N] double (as pf_hostio.cpp::pair_at forms it), the rooted tree (parent [2N-2], children [2N-2][3],
// -1 where absent, ascending), and for every directed subtree X (row e: below edge e; row 2N-3+e: beyond its parent end)
//   depth int16 [4N-6][2N-2]   every node's distance in edges from X's root node, -1 outside X (built on the host)
//   M     double [4N-6][N]     M[X][j] = sum_i w_X(i) d_ij, w = 2^-depth at use (ldexp: exact, cannot drift)
// and q double [2N-3][6] = d_AB, d_CD, d_A c1, d_A c2, d_B c1, d_B c2 of every edge, d_XY = numpy's pairwise sum over
// all j < N of w_Y(j) M[X][j] by one thread (pf_nj_host.h::pairwise_sum: the order depends on N alone).
//
// One step: eval (q of every edge, the two keys (delta, c, k) of every internal edge, the workgroup minima), move (the
// minimum; below THRESHOLD the swap on parent / children, else the source is done; the case of every row), update (depth
// and M of every row that contains the moved edge).  Steps run in rounds of ROUND_STEPS; every body returns at once for
// a done or flagged source.  A source done on the incrementally updated table gets depth rebuilt on the host and M from
// scratch (build_elem) and is evaluated once more: it is finished only if that table offers no move either, so the
// final q - lengths and tree_length - are those of bme.py's from-scratch table of the same topology, bit for bit.
//
// The update, case by case.  The move swaps s (block B) with x (block C, child of c); y (block D) is c's other child, A
// the rest beyond p.  A row X contains the edge iff depth[X][p] >= 0 and depth[X][c] >= 0; then X holds three of the
// four blocks whole and its root lies on the side of the fourth, Q.  With h = min(depth[X][p], depth[X][c]) before the
// move (Q in {A, B}: p comes first, h = depth[X][p]; Q in {C, D}: c comes first):
//   Q = A (s at h + 1):      B one edge down (+1), C one edge up (-1); p, c, D stay
//   Q = B (s outside or up): X now enters through c:  c -1, p +1, D -1, A +1; C stays
//   Q = C (x outside or up): X now enters through p:  p -1, c +1, A -1, D +1; B stays
//   Q = D (x at h + 1):      B -1, C +1; p, c, A stay
// A block P that moves by t edges has its leaves' weights multiplied by f = 2^-t, so M[X][j] += (f - 1) 2^-depth_X(root
// of P) M[P][j]; the roots of the moved blocks stand at h + 1 (f = 1/2) or h + 2 (f = 2), so every coefficient is
// + or - u, u = 2^-(h + 2): Q = A: -u M[B] + u M[C]; Q = B: -u M[A] + u M[D]; Q = C: u M[A] - u M[D]; Q = D: u M[B] - u
// M[C], added in that order.  The two rows of edge c itself do not contain the edge but change their members: below c
// stand B and D now (depth 1 + the block's own, M = M[B] / 2 + M[D] / 2), beyond c's parent end p, A and C (M = M[A] / 2 +
// M[C] / 2).  The rows of A, B, C and D neither contain the edge nor change, so they are read-only here; the case and h
// of every row are fixed by the move body before any depth changes, so nothing depends on arrival order.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pf_nj_host.h"

namespace pfbme {

constexpr double THRESHOLD = -1e-12;      // a move is performed iff delta < THRESHOLD
constexpr int ROUND_STEPS = 32;           // steps enqueued between two looks at the flags
constexpr int MAX_N = 16384;              // depth is int16: 2N - 3 < 32768
constexpr uint8_t ST_OK = 0, ST_NONFINITE = 1, ST_CAPPED = 2;

// a move and its value; ordered by (v, c, k)
struct Key { double v; int32_t c, k; };
PF_TAXA_HD inline Key key_none() { return Key{INFINITY, INT32_MAX, INT32_MAX}; }
PF_TAXA_HD inline bool key_less(const Key& x, const Key& y) {
    return x.v < y.v || (x.v == y.v && (x.c < y.c || (x.c == y.c && x.k < y.k)));
}

PF_TAXA_HD inline int64_t nodes_of(int N) { return 2 * (int64_t)N - 2; }
PF_TAXA_HD inline int64_t root_of(int N) { return 2 * (int64_t)N - 3; }        // the root node = the number of edges
PF_TAXA_HD inline int64_t rows_of(int N) { return 4 * (int64_t)N - 6; }
PF_TAXA_HD inline int64_t step_cap(int N) { return 16 * (int64_t)N; }

// what the move body decides and the update bodies read
struct Move { int32_t ok, c, p, s, x, y, arow; };

struct Args {
    const float* preds;     // [B][P_N]
    double* d;              // [B][N][N]
    int16_t* depth;         // [B][4N-6][2N-2]
    double* M;              // [B][4N-6][N]
    double* q;              // [B][2N-3][6]
    double* edge_len;       // [B][2N-3]
    Key* part;              // [B][part_cap]: the minimum of every workgroup of the evaluation
    int32_t* parent;        // [B][2N-2]
    int32_t* children;      // [B][2N-2][3]
    Move* move;             // [B]
    int16_t* rowh;          // [B][4N-6]
    int8_t* rowcase;        // [B][4N-6]: 0 = the row stays, 1 .. 4 = it contains the moved edge and Q is A .. D, 5 = the
                            // row below c, 6 = the row beyond c's parent end
    int32_t* steps;         // [B]
    uint8_t* done;          // [B]
    uint8_t* rebuild;       // [B]: build_elem forms M of this source
    uint8_t* status;        // [B]
    int N, part_cap;
    int64_t PN;
};

PF_TAXA_HD inline bool idle(const Args& a, size_t src) { return a.status[src] == ST_NONFINITE || a.done[src]; }
// 2^-dep (0 outside the subtree, dep < 0): exact either way - the device's ldexp is one instruction, the host's a
// library call, so a normal result is put together from its exponent there
PF_TAXA_HD inline double weight(int dep) {
    if (dep < 0) return 0.0;
#if !defined(__HIP_DEVICE_COMPILE__)
    if (dep <= 1022) {
        const uint64_t bits = (uint64_t)(1023 - dep) << 52;
        double w;
        memcpy(&w, &bits, sizeof w);
        return w;
    }
#endif
    return ldexp(1.0, -dep);
}
PF_TAXA_HD inline const int16_t* depth_row(const Args& a, size_t src, int64_t X) {
    return a.depth + ((int64_t)src * rows_of(a.N) + X) * nodes_of(a.N);
}
PF_TAXA_HD inline const double* M_row(const Args& a, size_t src, int64_t X) {
    return a.M + ((int64_t)src * rows_of(a.N) + X) * (int64_t)a.N;
}

// Thread `tid` of workgroup `wg` of `G`: the elements e = wg * threads + tid, + G * threads, ... of d; a NaN or an
// infinity flags the source.
PF_TAXA_HD inline void init_elems(const Args& a, size_t src, int wg, int G, int tid, int threads) {
    const int64_t N = a.N, NN = N * N;
    const float* preds = a.preds + src * (size_t)a.PN;
    double* d = a.d + src * (size_t)NN;
    bool bad = false;
    for (int64_t e = (int64_t)wg * threads + tid; e < NN; e += (int64_t)G * threads) {
        const int64_t i = e / N, j = e % N;
        if (i == j) { d[e] = 0.0; continue; }
        const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
        const float x = preds[lo * N - lo * (lo + 1) / 2 + (hi - lo - 1)];
        bad |= !(x - x == 0.0f);
        d[e] = (double)(x + 0.0f);
    }
    if (bad) a.status[src] = ST_NONFINITE;
}

// M[X][j] from scratch: i ascending, the product and the add rounded separately
PF_TAXA_HD inline void build_elem(const Args& a, size_t src, int64_t X, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!a.rebuild[src] || a.status[src] == ST_NONFINITE) return;
    const int64_t N = a.N;
    const int16_t* dep = depth_row(a, src, X);
    const double* d = a.d + (int64_t)src * N * N + j;
    double acc = 0.0;
    for (int64_t i = 0; i < N; ++i) {
        const double prod = weight(dep[i]) * d[i * N];
        acc += prod;
    }
    a.M[((int64_t)src * rows_of(a.N) + X) * N + j] = acc;
}

// Host only: build_elem for every j of row X at once, i outermost so that d is read along its rows.  Every M[X][j] sees
// the operations of build_elem in its order; an i outside X is skipped, which adds nothing (the sum starts at +0 and
// never becomes -0, so adding the +0 or -0 product of a zero weight leaves it as it is; the input is finite).
inline void build_row(const Args& a, size_t src, int64_t X) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!a.rebuild[src] || a.status[src] == ST_NONFINITE) return;
    const int64_t N = a.N;
    const int16_t* dep = depth_row(a, src, X);
    const double* d = a.d + (int64_t)src * N * N;
    double* acc = a.M + ((int64_t)src * rows_of(a.N) + X) * N;
    for (int64_t j = 0; j < N; ++j) acc[j] = 0.0;
    for (int64_t i = 0; i < N; ++i) {
        if (dep[i] < 0) continue;
        const double w = weight(dep[i]);
        const double* di = d + i * N;
        for (int64_t j = 0; j < N; ++j) {
            const double prod = w * di[j];
            acc[j] += prod;
        }
    }
}

// what stands around edge e: its parent p, its sibling s (B), A's row, and e's children (-1 for a leaf)
struct Quartet { int32_t p, s, arow, c1, c2; };
PF_TAXA_HD inline Quartet quartet_of(const Args& a, size_t src, int e) {
    const int64_t nodes = nodes_of(a.N), root = root_of(a.N);
    const int32_t* parent = a.parent + (int64_t)src * nodes;
    const int32_t* children = a.children + (int64_t)src * nodes * 3;
    Quartet t;
    t.p = parent[e];
    const int32_t* ch = children + (int64_t)t.p * 3;
    if (t.p == root) {
        t.s = ch[0] == e ? ch[1] : ch[0];
        t.arow = ch[2] == e ? ch[1] : ch[2];
    } else {
        t.s = ch[0] == e ? ch[1] : ch[0];
        t.arow = (int32_t)(root + t.p);
    }
    t.c1 = children[(int64_t)e * 3];
    t.c2 = children[(int64_t)e * 3 + 1];
    return t;
}

PF_TAXA_HD inline double d_xy(const Args& a, size_t src, int64_t X, int64_t Y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double* m = M_row(a, src, X);
    const int16_t* dep = depth_row(a, src, Y);
    return pfnj::pairwise_sum([&](int j) { return weight(dep[j]) * m[j]; }, a.N);
}

// element qi of edge e's q (a leaf edge has d_AB, d_A e and d_B e only)
PF_TAXA_HD inline double eval_q(const Args& a, size_t src, int e, int qi) {
    const Quartet t = quartet_of(a, src, e);
    const bool leaf = t.c1 < 0;
    if (leaf && (qi & 1)) return 0.0;
    const int32_t c1 = leaf ? e : t.c1, c2 = t.c2;
    // one call site, so that the device holds one copy of the sum
    const int64_t X = qi == 1 ? c1 : qi >= 4 ? t.s : t.arow;
    const int64_t Y = qi == 0 ? t.s : (qi == 2 || qi == 4) ? c1 : c2;
    return d_xy(a, src, X, Y);
}

PF_TAXA_HD inline Key key_of(int N, int e, int k, const double* q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (e < N) return key_none();
    const double ab_cd = q[0] + q[1];
    const double v = k == 0 ? 0.5 * ((q[2] + q[5]) - ab_cd) : 0.5 * ((q[3] + q[4]) - ab_cd);
    return Key{v, e, k};
}

// The evaluation's workgroup `wg` covers edges wg * epg .. wg * epg + epg - 1.  First every thread the elements tid,
// tid + threads, ... of their q [epg][6] (into lq, the workgroup's scratch, and the table); after a barrier every thread
// the minimum of the keys tid, tid + threads, ... of [epg][2].
PF_TAXA_HD inline void eval_q_thread(const Args& a, size_t src, int wg, int epg, int tid, int threads, double* lq) {
    if (idle(a, src)) return;
    const int64_t root = root_of(a.N);
    for (int i = tid; i < epg * 6; i += threads) {
        const int64_t e = (int64_t)wg * epg + i / 6;
        if (e >= root) break;
        const double v = eval_q(a, src, (int)e, i % 6);
        lq[i] = v;
        a.q[((int64_t)src * root + e) * 6 + i % 6] = v;
    }
}
PF_TAXA_HD inline Key eval_key_thread(const Args& a, size_t src, int wg, int epg, int tid, int threads, const double* lq) {
    Key best = key_none();
    if (idle(a, src)) return best;
    const int64_t root = root_of(a.N);
    for (int i = tid; i < epg * 2; i += threads) {
        const int64_t e = (int64_t)wg * epg + i / 2;
        if (e >= root) break;
        const Key k = key_of(a.N, (int)e, i % 2, lq + (i / 2) * 6);
        if (key_less(k, best)) best = k;
    }
    return best;
}

// One step of the minimum of keys[0 .. threads) in a workgroup (a barrier stands between two steps), as
// pfnj::reduce_step; the first s is pfnj::reduce_first_step(threads).
PF_TAXA_HD inline void reduce_step(Key* keys, int tid, int s, int threads) {
    if (tid < s && tid + s < threads && key_less(keys[tid + s], keys[tid])) keys[tid] = keys[tid + s];
}

// thread `tid` of the move's one workgroup: the minimum of the partial minima tid, tid + threads, ... of G
PF_TAXA_HD inline Key move_thread_key(const Args& a, size_t src, int G, int tid, int threads) {
    Key best = key_none();
    if (idle(a, src)) return best;
    const Key* part = a.part + src * (size_t)a.part_cap;
    for (int g = tid; g < G; g += threads)
        if (key_less(part[g], best)) best = part[g];
    return best;
}

// One thread: no qualifying move - the source is done; the cap reached - done and capped; else the swap on parent /
// children.  Always writes the source's Move (ok = 0: nothing moved).
PF_TAXA_HD inline Move move_decide(const Args& a, size_t src, Key best) {
    Move m{0, 0, 0, 0, 0, 0, 0};
    if (idle(a, src)) { a.move[src] = m; return m; }
    const int64_t nodes = nodes_of(a.N), root = root_of(a.N);
    if (!(best.v < THRESHOLD)) { a.done[src] = 1; a.move[src] = m; return m; }
    if (a.steps[src] >= step_cap(a.N)) { a.status[src] = ST_CAPPED; a.done[src] = 1; a.move[src] = m; return m; }
    if (best.c < a.N || best.c >= root || best.k < 0 || best.k > 1) {       // never with finite input
        a.status[src] = ST_NONFINITE; a.move[src] = m; return m;
    }
    int32_t* parent = a.parent + (int64_t)src * nodes;
    int32_t* children = a.children + (int64_t)src * nodes * 3;
    const Quartet t = quartet_of(a, src, best.c);
    m.ok = 1; m.c = best.c; m.p = t.p; m.s = t.s; m.arow = t.arow;
    m.x = best.k == 0 ? t.c1 : t.c2;
    m.y = best.k == 0 ? t.c2 : t.c1;
    parent[m.s] = m.c;
    parent[m.x] = m.p;
    int32_t* cc = children + (int64_t)m.c * 3;
    cc[0] = m.s < m.y ? m.s : m.y;
    cc[1] = m.s < m.y ? m.y : m.s;
    int32_t* pc = children + (int64_t)m.p * 3;
    const int np = m.p == root ? 3 : 2;
    for (int i = 0; i < np; ++i) if (pc[i] == m.s) pc[i] = m.x;
    for (int i = 1; i < np; ++i)                                             // two or three entries: insertion sort
        for (int j = i; j > 0 && pc[j] < pc[j - 1]; --j) { const int32_t tmp = pc[j]; pc[j] = pc[j - 1]; pc[j - 1] = tmp; }
    a.steps[src] += 1;
    a.move[src] = m;
    return m;
}

// thread `tid` of the move's workgroup after move_decide: the case and h of rows tid, tid + threads, ... (depth is
// still the table before the move)
PF_TAXA_HD inline void move_rowcase(const Args& a, size_t src, const Move& m, int tid, int threads) {
    if (!m.ok) return;
    const int64_t rows = rows_of(a.N);
    for (int64_t X = tid; X < rows; X += threads) {
        const int16_t* dep = depth_row(a, src, X);
        const int dp = dep[m.p], dc = dep[m.c];
        int8_t rc = 0;
        int16_t h = 0;
        if (dp >= 0 && dc >= 0) {
            if (dp < dc) { rc = dep[m.s] == dp + 1 ? 1 : 2; h = (int16_t)dp; }
            else { rc = dep[m.x] == dc + 1 ? 4 : 3; h = (int16_t)dc; }
        }
        if (X == m.c) rc = 5;
        if (X == root_of(a.N) + m.c) rc = 6;
        a.rowcase[(int64_t)src * rows + X] = rc;
        a.rowh[(int64_t)src * rows + X] = h;
    }
}

// Element (X, v) of the update, one thread each: depth[X][v] for every node v, and M[X][v] for a leaf v.
PF_TAXA_HD inline void update_elem(const Args& a, size_t src, int64_t X, int v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const Move m = a.move[src];
    if (!m.ok) return;
    const int64_t rows = rows_of(a.N), nodes = nodes_of(a.N);
    const int rc = a.rowcase[(int64_t)src * rows + X];
    if (!rc) return;
    if (rc >= 5) {                                   // the rows of edge c: two blocks, each one edge below the root
        const int64_t r1 = rc == 5 ? m.s : m.arow, r2 = rc == 5 ? m.y : m.x;
        if (v < a.N) {
            const double t1 = 0.5 * M_row(a, src, r1)[v];
            const double t2 = 0.5 * M_row(a, src, r2)[v];
            a.M[((int64_t)src * rows + X) * (int64_t)a.N + v] = t1 + t2;
        }
        const int d1 = depth_row(a, src, r1)[v], d2 = depth_row(a, src, r2)[v];
        a.depth[((int64_t)src * rows + X) * nodes + v] =
            (int16_t)(v == (rc == 5 ? m.c : m.p) ? 0 : d1 >= 0 ? d1 + 1 : d2 >= 0 ? d2 + 1 : -1);
        return;
    }
    if (v < a.N) {
        const double u = ldexp(1.0, -((int)a.rowh[(int64_t)src * rows + X] + 2));
        const int64_t r1 = rc == 1 || rc == 4 ? m.s : m.arow, r2 = rc == 1 || rc == 4 ? m.x : m.y;
        const double c1 = rc <= 2 ? -u : u, c2 = rc <= 2 ? u : -u;
        double* dst = a.M + ((int64_t)src * rows + X) * (int64_t)a.N + v;
        const double t1 = c1 * M_row(a, src, r1)[v];
        const double t2 = c2 * M_row(a, src, r2)[v];
        *dst = (*dst + t1) + t2;
    }
    int16_t* dep = a.depth + ((int64_t)src * rows + X) * nodes + v;
    if (*dep < 0) return;
    // the block of v: p, c, B, C, D, else A
    int delta;
    if (v == m.p) delta = rc == 2 ? 1 : rc == 3 ? -1 : 0;
    else if (v == m.c) delta = rc == 2 ? -1 : rc == 3 ? 1 : 0;
    else if (depth_row(a, src, m.s)[v] >= 0) delta = rc == 1 ? 1 : rc == 4 ? -1 : 0;
    else if (depth_row(a, src, m.x)[v] >= 0) delta = rc == 1 ? -1 : rc == 4 ? 1 : 0;
    else if (depth_row(a, src, m.y)[v] >= 0) delta = rc == 2 ? -1 : rc == 3 ? 1 : 0;
    else delta = rc == 2 ? 1 : rc == 3 ? -1 : 0;
    *dep = (int16_t)(*dep + delta);
}

// the balanced length of edge e from q
PF_TAXA_HD inline void edge_length(const Args& a, size_t src, int e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (a.status[src] == ST_NONFINITE) return;
    const int64_t root = root_of(a.N);
    const double* q = a.q + ((int64_t)src * root + e) * 6;
    a.edge_len[(int64_t)src * root + e] =
        e < a.N ? 0.5 * ((q[2] + q[4]) - q[0]) : 0.25 * (((q[2] + q[3]) + q[4]) + q[5]) - 0.5 * (q[0] + q[1]);
}

// ---- host only: the tree of a join table, the depth table, the join table of a tree --------------------------------

// parent [2N-2] / children [2N-2][3] of the start table (lengths are not needed); false: not a valid join table
inline bool tree_of_joins(const int32_t* slots, int N, int32_t* parent, int32_t* children) {
    const int64_t nodes = nodes_of(N), root = root_of(N);
    std::fill(parent, parent + nodes, -1);
    std::fill(children, children + nodes * 3, -1);
    std::vector<int32_t> cluster((size_t)N);
    for (int i = 0; i < N; ++i) cluster[(size_t)i] = i;
    auto adopt = [&](int64_t node, int32_t* kids, int n) {
        std::sort(kids, kids + n);
        for (int i = 0; i < n; ++i) { children[node * 3 + i] = kids[i]; parent[kids[i]] = (int32_t)node; }
    };
    for (int t = 0; t < N - 3; ++t) {
        const int32_t sa = slots[2 * t], sb = slots[2 * t + 1];
        if (sa < 0 || sa >= N || sb < 0 || sb >= N || sa == sb || cluster[(size_t)sa] < 0 || cluster[(size_t)sb] < 0) return false;
        int32_t kids[2] = {cluster[(size_t)sa], cluster[(size_t)sb]};
        adopt(N + t, kids, 2);
        cluster[(size_t)sa] = N + t;
        cluster[(size_t)sb] = -1;
    }
    const int32_t* last = slots + 2 * ((int64_t)N - 3);
    for (int i = 0; i < 3; ++i) if (last[i] < 0 || last[i] >= N || cluster[(size_t)last[i]] < 0) return false;
    if (last[0] == last[1] || last[0] == last[2] || last[1] == last[2]) return false;
    int32_t kids[3] = {cluster[(size_t)last[0]], cluster[(size_t)last[1]], cluster[(size_t)last[2]]};
    adopt(root, kids, 3);
    return true;
}

// the nodes parents before children, from the root
inline void top_down(const int32_t* children, int N, std::vector<int32_t>& order) {
    order.clear();
    order.push_back((int32_t)root_of(N));
    for (size_t at = 0; at < order.size(); ++at)
        for (int i = 0; i < 3; ++i) {
            const int32_t c = children[(int64_t)order[at] * 3 + i];
            if (c >= 0) order.push_back(c);
        }
}

// depth [4N-6][2N-2] of a tree (bme.py::Tree.depths): O(N^2)
inline void build_depth(const int32_t* parent, const int32_t* children, int N, int16_t* depth) {
    const int64_t nodes = nodes_of(N), root = root_of(N), rows = rows_of(N);
    std::fill(depth, depth + rows * nodes, (int16_t)-1);
    std::vector<int32_t> order;
    top_down(children, N, order);
    auto hang = [&](int64_t row, int64_t under) {
        int16_t* dst = depth + row * nodes;
        const int16_t* src = depth + under * nodes;
        for (int64_t v = 0; v < nodes; ++v) if (src[v] >= 0) dst[v] = (int16_t)(src[v] + 1);
    };
    for (size_t at = order.size(); at-- > 1;) {
        const int64_t v = order[at];
        depth[v * nodes + v] = 0;
        for (int i = 0; i < 3; ++i) if (children[v * 3 + i] >= 0) hang(v, children[v * 3 + i]);
    }
    for (size_t at = 1; at < order.size(); ++at) {
        const int64_t v = order[at], p = parent[v];
        depth[(root + v) * nodes + p] = 0;
        for (int i = 0; i < 3; ++i) {
            const int32_t c = children[p * 3 + i];
            if (c >= 0 && c != v) hang(root + v, c);
        }
        if (p != root) hang(root + v, root + p);
    }
}

// The join table of a tree and its edge lengths (bme.py::joins_of_tree): internal nodes by (leaves, smallest leaf), a
// cluster's slot its smallest leaf, then the root's children by slot.
inline void joins_of_tree(const int32_t* children, const double* edge_len, int N, int32_t* slots, double* lengths) {
    const int64_t nodes = nodes_of(N), root = root_of(N);
    std::vector<int32_t> order, size((size_t)nodes, 1), low((size_t)nodes), inner;
    for (int64_t v = 0; v < nodes; ++v) low[(size_t)v] = (int32_t)v;
    top_down(children, N, order);
    for (size_t at = order.size(); at-- > 0;) {
        const int64_t v = order[at];
        if (v < N) continue;
        int32_t sz = 0, lo = INT32_MAX;
        for (int i = 0; i < 3; ++i) {
            const int32_t c = children[v * 3 + i];
            if (c >= 0) { sz += size[(size_t)c]; lo = std::min(lo, low[(size_t)c]); }
        }
        size[(size_t)v] = sz; low[(size_t)v] = lo;
    }
    for (int64_t v = N; v < root; ++v) inner.push_back((int32_t)v);
    std::sort(inner.begin(), inner.end(), [&](int32_t x, int32_t y) {
        return size[(size_t)x] != size[(size_t)y] ? size[(size_t)x] < size[(size_t)y] : low[(size_t)x] < low[(size_t)y];
    });
    inner.push_back((int32_t)root);
    size_t at = 0;
    for (int32_t v : inner) {
        int32_t kids[3];
        int n = 0;
        for (int i = 0; i < 3; ++i) if (children[(int64_t)v * 3 + i] >= 0) kids[n++] = children[(int64_t)v * 3 + i];
        std::sort(kids, kids + n, [&](int32_t x, int32_t y) { return low[(size_t)x] < low[(size_t)y]; });
        for (int i = 0; i < n; ++i, ++at) { slots[at] = low[(size_t)kids[i]]; lengths[at] = edge_len[kids[i]]; }
    }
}

// the sum of the edge lengths in edge order
inline double tree_length_of(const double* edge_len, int N) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double total = 0.0;
    for (int64_t e = 0; e < root_of(N); ++e) total += edge_len[e];
    return total;
}

// What the host decides between two rounds, for the device and the serial driver alike.  `fresh[src]` = the steps at
// the source's last from-scratch table.  Returns true when every source is finished; otherwise `rebuild` marks the
// sources whose depth (rebuilt here, in the host copy) and M (build_elem) start over, with done cleared.  `resumes`,
// when not NULL, counts the times a from-scratch table offered a move that the updated one had not.
inline bool between_rounds(int B, int N, const int32_t* parent, const int32_t* children, const int32_t* steps, uint8_t* done,
                           const uint8_t* status, uint8_t* rebuild, int32_t* fresh, int16_t* depth, int64_t* resumes = nullptr) {
    const int64_t nodes = nodes_of(N), rows = rows_of(N);
    bool all = true;
    for (int b = 0; b < B; ++b) {
        rebuild[b] = 0;
        if (status[b] == ST_NONFINITE) continue;
        if (!done[b]) { all = false; continue; }
        if (steps[b] == fresh[b]) continue;
        if (resumes && fresh[b] > 0) ++*resumes;
        build_depth(parent + b * nodes, children + b * nodes * 3, N, depth + b * rows * nodes);
        rebuild[b] = 1; done[b] = 0; fresh[b] = steps[b];
        all = false;
    }
    return all;
}

// the results of one source: its join table, steps, tree length and status (a flagged source: zeros)
inline void result_of(int N, const int32_t* children, const double* edge_len, int32_t steps, uint8_t status, int32_t* slots,
                      double* lengths, int32_t* steps_out, double* tree_length, uint8_t* status_out) {
    const size_t T = (size_t)pfnj::table_len(N);
    *status_out = status;
    if (status == ST_NONFINITE) {
        std::fill(slots, slots + T, 0); std::fill(lengths, lengths + T, 0.0);
        *steps_out = 0; *tree_length = 0.0;
        return;
    }
    joins_of_tree(children, edge_len, N, slots, lengths);
    *steps_out = steps;
    *tree_length = tree_length_of(edge_len, N);
}

// The state of B sources on the host, exactly sized, and the serial run of the bodies in the order the launches of
// pf_bme.hip.h give them: workgroups of `threads` threads, `epg` edges per workgroup of the evaluation.
struct Serial {
    int B, N;
    std::vector<double> d, M, q, edge_len;
    std::vector<int16_t> depth, rowh;
    std::vector<Key> part;
    std::vector<int32_t> parent, children, steps, fresh;
    std::vector<Move> move;
    std::vector<int8_t> rowcase;
    std::vector<uint8_t> done, rebuild, status;
    int64_t resumes = 0;          // from-scratch tables that offered a move the updated table had not
    Args a{};

    // false: an invalid start table (status is not touched)
    bool setup(const float* preds, const int32_t* start_slots, int B_, int N_, int epg) {
        B = B_; N = N_;
        const size_t b = (size_t)B, n = (size_t)N, nodes = (size_t)nodes_of(N), rows = (size_t)rows_of(N), root = (size_t)root_of(N);
        const size_t G = (root + (size_t)epg - 1) / (size_t)epg;
        d.assign(b * n * n, 0.0); M.assign(b * rows * n, 0.0); q.assign(b * root * 6, 0.0); edge_len.assign(b * root, 0.0);
        depth.assign(b * rows * nodes, -1); rowh.assign(b * rows, 0); part.assign(b * G, key_none());
        parent.assign(b * nodes, -1); children.assign(b * nodes * 3, -1); steps.assign(b, 0); fresh.assign(b, 0);
        move.assign(b, Move{0, 0, 0, 0, 0, 0, 0}); rowcase.assign(b * rows, 0);
        done.assign(b, 0); rebuild.assign(b, 1); status.assign(b, ST_OK);
        for (size_t s = 0; s < b; ++s) {
            if (!tree_of_joins(start_slots + s * (size_t)pfnj::table_len(N), N, &parent[s * nodes], &children[s * nodes * 3])) return false;
            build_depth(&parent[s * nodes], &children[s * nodes * 3], N, &depth[s * rows * nodes]);
        }
        a.preds = preds; a.d = d.data(); a.depth = depth.data(); a.M = M.data(); a.q = q.data(); a.edge_len = edge_len.data();
        a.part = part.data(); a.parent = parent.data(); a.children = children.data(); a.move = move.data(); a.rowh = rowh.data();
        a.rowcase = rowcase.data(); a.steps = steps.data(); a.done = done.data(); a.rebuild = rebuild.data(); a.status = status.data();
        a.N = N; a.part_cap = (int)G; a.PN = (int64_t)N * (N - 1) / 2;
        return true;
    }

    // rows_at_once: M is built row by row (build_row) instead of element by element (build_elem): the same bits
    void run(int threads, int epg, int init_groups, bool rows_at_once = false) {
        const int64_t rows = rows_of(N), nodes = nodes_of(N), root = root_of(N);
        const int G = a.part_cap;
        std::vector<Key> keys((size_t)threads);
        std::vector<double> lq((size_t)epg * 6);
        auto reduce = [&] {
            for (int s = pfnj::reduce_first_step(threads); s > 0; s >>= 1)
                for (int tid = 0; tid < threads; ++tid) reduce_step(keys.data(), tid, s, threads);
        };
        for (size_t src = 0; src < (size_t)B; ++src)
            for (int wg = 0; wg < init_groups; ++wg)
                for (int tid = 0; tid < threads; ++tid) init_elems(a, src, wg, init_groups, tid, threads);
        for (;;) {
            for (size_t src = 0; src < (size_t)B; ++src)
                for (int64_t X = 0; X < rows; ++X) {
                    if (rows_at_once) { build_row(a, src, X); continue; }
                    for (int j = 0; j < N; ++j) build_elem(a, src, X, j);
                }
            for (int step = 0; step < ROUND_STEPS; ++step) {
                for (size_t src = 0; src < (size_t)B; ++src)
                    for (int wg = 0; wg < G; ++wg) {
                        for (int tid = 0; tid < threads; ++tid) eval_q_thread(a, src, wg, epg, tid, threads, lq.data());
                        for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = eval_key_thread(a, src, wg, epg, tid, threads, lq.data());
                        reduce();
                        part[src * (size_t)G + (size_t)wg] = keys[0];
                    }
                for (size_t src = 0; src < (size_t)B; ++src) {
                    for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = move_thread_key(a, src, G, tid, threads);
                    reduce();
                    const Move m = move_decide(a, src, keys[0]);
                    for (int tid = 0; tid < threads; ++tid) move_rowcase(a, src, m, tid, threads);
                }
                for (size_t src = 0; src < (size_t)B; ++src) {
                    if (!move[src].ok) continue;                     // (every element returns at once)
                    for (int64_t X = 0; X < rows; ++X) {
                        if (!rowcase[src * (size_t)rows + (size_t)X]) continue;
                        for (int v = 0; v < (int)nodes; ++v) update_elem(a, src, X, v);
                    }
                }
            }
            if (between_rounds(B, N, parent.data(), children.data(), steps.data(), done.data(), status.data(), rebuild.data(),
                               fresh.data(), depth.data(), &resumes))
                break;
        }
        for (size_t src = 0; src < (size_t)B; ++src)
            for (int e = 0; e < (int)root; ++e) edge_length(a, src, e);
    }

    void result(size_t src, int32_t* slots, double* lengths, int32_t* steps_out, double* tree_length, uint8_t* status_out) const {
        result_of(N, &children[src * (size_t)nodes_of(N) * 3], &edge_len[src * (size_t)root_of(N)], steps[src], status[src], slots,
                  lengths, steps_out, tree_length, status_out);
    }
};

}  // namespace pfbme
