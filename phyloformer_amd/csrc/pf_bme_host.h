// Balanced minimum-evolution NNI refinement (pf_bme_nni, pf_bme_nni_device, pf_bme_nni_host, pf_bme_newick_n; DESIGN.md
// section 21; the balanced SPR search of section 22 follows it below and shares its tree, rows and tables): the bodies
// of the kernels of pf_bme.hip.h as functions of (source, workgroup, thread), the host-side tree bookkeeping, the lists
// of the arrays of both states (state_arrays, spr_state_arrays: sizes, device spans and host allocations all come from
// them), and the serial drivers that run the same bodies without a device.  Plain C++, no HIP:
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

constexpr int THREADS = 256;               // every workgroup of the device
constexpr int EVAL_EDGES = 32;             // edges per workgroup of k_bme_eval: 192 sums, 64 keys
constexpr int SPR_EVAL_EDGES = THREADS;    // target edges per workgroup of k_bme_spr_eval: one per thread

// A move and its value, ordered by (v, a, b).  Balanced NNI: a = the internal edge c, b = which of its children (k).
// Balanced SPR: a = the row of the pruned subtree S, b = the target edge.
using pfnj::Key;
using pfnj::key_less;
using pfnj::key_none;

PF_TAXA_HD inline int64_t nodes_of(int N) { return 2 * (int64_t)N - 2; }
PF_TAXA_HD inline int64_t root_of(int N) { return 2 * (int64_t)N - 3; }        // the root node = the number of edges
PF_TAXA_HD inline int64_t rows_of(int N) { return 4 * (int64_t)N - 6; }
PF_TAXA_HD inline int64_t step_cap(int N) { return 16 * (int64_t)N; }
// workgroups of an evaluation of `epg` edges each
PF_TAXA_HD inline int eval_groups(int N, int epg) { return (int)((root_of(N) + epg - 1) / epg); }

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

// balanced SPR (the section further down): balanced NNI's arguments and its own on top
struct SprArgs {
    Args b;                 // d, depth, M, q, edge_len, part, parent, children, steps, done (0), rebuild, status
    double* T;              // [B][4N-6][4N-6]
    Key* spart;             // [B][spart_cap]: the minimum key (dL, S row, target edge) of every workgroup of the evaluation
    int32_t* tin;           // [B][2N-2]: entry time of every node
    int32_t* tout;          // [B][2N-2]: the last entry time in its subtree
    int32_t* ndepth;        // [B][2N-2]: edges from the root
    int32_t* path;          // [B][2N-2]: u_1 .. u_i, t of the move
    uint8_t* sdone;         // [B]
    int64_t cap;            // moves after which a source is capped (step_cap(N) but for tests)
    int spart_cap, epg;     // epg: target edges per workgroup of the evaluation
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
// infinity flags the source.  (The statements of pfnj::init_elems: see the note there.)
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
PF_TAXA_HD inline Quartet quartet_of(const int32_t* parent, const int32_t* children, int64_t root, int e) {
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
PF_TAXA_HD inline Quartet quartet_of(const Args& a, size_t src, int e) {
    const int64_t nodes = nodes_of(a.N);
    return quartet_of(a.parent + (int64_t)src * nodes, a.children + (int64_t)src * nodes * 3, root_of(a.N), e);
}

// bme.py::Tree.swap: the sibling s of internal edge c and child x of c change places (y is c's other child)
PF_TAXA_HD inline void swap_blocks(int32_t* parent, int32_t* children, int64_t root, int32_t c, int32_t p, int32_t s, int32_t x, int32_t y) {
    parent[s] = c;
    parent[x] = p;
    int32_t* cc = children + (int64_t)c * 3;
    cc[0] = s < y ? s : y;
    cc[1] = s < y ? y : s;
    int32_t* pc = children + (int64_t)p * 3;
    const int np = p == root ? 3 : 2;
    for (int i = 0; i < np; ++i) if (pc[i] == s) pc[i] = x;
    for (int i = 1; i < np; ++i)                                             // two or three entries: insertion sort
        for (int j = i; j > 0 && pc[j] < pc[j - 1]; --j) { const int32_t tmp = pc[j]; pc[j] = pc[j - 1]; pc[j - 1] = tmp; }
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
    return Key{v, e, k};                                        // (value, edge, child)
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
    if (best.a < a.N || best.a >= root || best.b < 0 || best.b > 1) {       // (edge, child); never with finite input
        a.status[src] = ST_NONFINITE; a.move[src] = m; return m;
    }
    int32_t* parent = a.parent + (int64_t)src * nodes;
    int32_t* children = a.children + (int64_t)src * nodes * 3;
    const Quartet t = quartet_of(a, src, best.a);
    m.ok = 1; m.c = best.a; m.p = t.p; m.s = t.s; m.arow = t.arow;
    m.x = best.b == 0 ? t.c1 : t.c2;
    m.y = best.b == 0 ? t.c2 : t.c1;
    swap_blocks(parent, children, root, m.c, m.p, m.s, m.x, m.y);
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

// The start tables and the results of a call (pf_bme_nni, pf_bme_spr) as the caller holds them, `u`, or - the device
// forms - their mirror on the host, `s`: the search reads and writes them on the host.
struct Tables { const int32_t* start; int32_t *slots, *steps; double *lengths, *tree_length; uint8_t* status; };
template <class V>
inline void mirror_arrays(V& v, Tables& s, const Tables& u, size_t B, int N) {
    const size_t T = (size_t)pfnj::table_len(N);
    v.in(s.start, u.start, B * T);
    v.out(s.slots, u.slots, B * T);
    v.out(s.steps, u.steps, B);
    v.out(s.lengths, u.lengths, B * T);
    v.out(s.tree_length, u.tree_length, B);
    v.out(s.status, u.status, B);
}

// ---- host only: the arrays of the state, listed once (the visitors and the padding rule: pf_nj_host.h) --------------

// the scalars of `a`; the arrays follow by state_arrays / spr_state_arrays
inline Args args_of(const float* preds, int N, int part_cap) {
    Args a{};
    a.preds = preds; a.N = N; a.part_cap = part_cap; a.PN = (int64_t)N * (N - 1) / 2;
    return a;
}

// balanced NNI
template <class V>
inline void state_arrays(V& v, Args& a, size_t B) {
    const size_t n = (size_t)a.N, nodes = (size_t)nodes_of(a.N), rows = (size_t)rows_of(a.N), root = (size_t)root_of(a.N);
    v(a.d, B * n * n);
    v(a.M, B * rows * n);
    v(a.q, B * root * 6);
    v(a.edge_len, B * root);
    v(a.part, B * (size_t)a.part_cap);
    v(a.move, B);
    v(a.parent, B * nodes);
    v(a.children, B * nodes * 3);
    v(a.steps, B);
    v(a.depth, B * rows * nodes);
    v(a.rowh, B * rows);
    v(a.rowcase, B * rows);
    v.flags(B, {&a.done, &a.rebuild, &a.status});
}

// balanced SPR: balanced NNI's arrays that the search shares (no move, rowh, rowcase), T, its partial minima, the
// numbering and the path
template <class V>
inline void spr_state_arrays(V& v, SprArgs& s, size_t B) {
    Args& a = s.b;
    const size_t n = (size_t)a.N, nodes = (size_t)nodes_of(a.N), rows = (size_t)rows_of(a.N), root = (size_t)root_of(a.N);
    v(a.d, B * n * n);
    v(a.M, B * rows * n);
    v(a.q, B * root * 6);
    v(a.edge_len, B * root);
    v(s.T, B * rows * rows);
    v(a.part, B * (size_t)a.part_cap);
    v(s.spart, B * (size_t)s.spart_cap);
    v(a.parent, B * nodes);
    v(a.children, B * nodes * 3);
    v(s.tin, B * nodes);
    v(s.tout, B * nodes);
    v(s.ndepth, B * nodes);
    v(s.path, B * nodes);
    v(a.steps, B);
    v(a.depth, B * rows * nodes);
    v.flags(B, {&a.done, &a.rebuild, &a.status, &s.sdone});
}

// the scalars of the search
inline SprArgs spr_args_of(const float* preds, int N, int part_cap, int epg, int64_t cap) {
    SprArgs s{};
    s.b = args_of(preds, N, part_cap);
    s.cap = cap; s.epg = epg;
    s.spart_cap = (int)(rows_of(N) * eval_groups(N, epg));
    return s;
}

// bytes of one source's state on the device, and the state of B sources carved from `ws` (8-byte aligned, B times
// those bytes): array after array, each [B][its share], so that a source's rows are contiguous
inline size_t state_bytes(int N) {
    Args a = args_of(nullptr, N, eval_groups(N, EVAL_EDGES));
    return pfspan::measure([&](auto& v) { state_arrays(v, a, 1); });
}
inline Args carve(char* ws, const float* preds, int B, int N) {
    Args a = args_of(preds, N, eval_groups(N, EVAL_EDGES));
    pfspan::carve(ws, [&](auto& v) { state_arrays(v, a, (size_t)B); });
    return a;
}
inline size_t spr_state_bytes(int N) {
    SprArgs s = spr_args_of(nullptr, N, eval_groups(N, EVAL_EDGES), SPR_EVAL_EDGES, 0);
    return pfspan::measure([&](auto& v) { spr_state_arrays(v, s, 1); });
}
inline SprArgs carve_spr(char* ws, const float* preds, int B, int N, int64_t cap) {
    SprArgs s = spr_args_of(preds, N, eval_groups(N, EVAL_EDGES), SPR_EVAL_EDGES, cap > 0 ? cap : step_cap(N));
    pfspan::carve(ws, [&](auto& v) { spr_state_arrays(v, s, (size_t)B); });
    return s;
}

// What the two serial drivers share: the state of B sources on the host, one exactly sized allocation per array, the
// start trees, the distances and the results.  `a` is the state of both; balanced NNI uses nothing else of `s`.
struct SerialBase {
    int B = 0, N = 0;
    pfnj::Allocate mem;
    SprArgs s{};
    Args& a = s.b;

    SerialBase() = default;
    SerialBase(const SerialBase&) = delete;

    // after the arrays: every source's tree and rebuild = 1; false: an invalid start table
    bool start_trees(const int32_t* start_slots) {
        const size_t nodes = (size_t)nodes_of(N);
        std::fill(a.rebuild, a.rebuild + B, (uint8_t)1);
        for (size_t src = 0; src < (size_t)B; ++src)
            if (!tree_of_joins(start_slots + src * (size_t)pfnj::table_len(N), N, a.parent + src * nodes, a.children + src * nodes * 3))
                return false;
        return true;
    }

    void init(int threads, int init_groups) {
        for (size_t src = 0; src < (size_t)B; ++src)
            for (int wg = 0; wg < init_groups; ++wg)
                for (int tid = 0; tid < threads; ++tid) init_elems(a, src, wg, init_groups, tid, threads);
    }

    void result(size_t src, int32_t* slots, double* lengths, int32_t* steps_out, double* tree_length, uint8_t* status_out) const {
        result_of(N, a.children + src * (size_t)nodes_of(N) * 3, a.edge_len + src * (size_t)root_of(N), a.steps[src], a.status[src],
                  slots, lengths, steps_out, tree_length, status_out);
    }
};

// The serial run of balanced NNI's bodies in the order the launches of pf_bme.hip.h give them: workgroups of `threads`
// threads, `epg` edges per workgroup of the evaluation.
struct Serial : SerialBase {
    std::vector<int32_t> fresh;
    int64_t resumes = 0;          // from-scratch tables that offered a move the updated table had not

    // false: an invalid start table (status is not touched)
    bool setup(const float* preds, const int32_t* start_slots, int B_, int N_, int epg) {
        B = B_; N = N_;
        a = args_of(preds, N, eval_groups(N, epg));
        state_arrays(mem, a, (size_t)B);
        fresh.assign((size_t)B, 0);
        if (!start_trees(start_slots)) return false;
        const size_t nodes = (size_t)nodes_of(N), rows = (size_t)rows_of(N);
        for (size_t src = 0; src < (size_t)B; ++src)
            build_depth(a.parent + src * nodes, a.children + src * nodes * 3, N, a.depth + src * rows * nodes);
        return true;
    }

    // rows_at_once: M is built row by row (build_row) instead of element by element (build_elem): the same bits
    void run(int threads, int epg, int init_groups, bool rows_at_once = false) {
        const int64_t rows = rows_of(N), nodes = nodes_of(N), root = root_of(N);
        const int G = a.part_cap;
        std::vector<Key> keys((size_t)threads);
        std::vector<double> lq((size_t)epg * 6);
        init(threads, init_groups);
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
                        pfnj::reduce_keys_serial(keys.data(), threads);
                        a.part[src * (size_t)G + (size_t)wg] = keys[0];
                    }
                for (size_t src = 0; src < (size_t)B; ++src) {
                    for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = move_thread_key(a, src, G, tid, threads);
                    pfnj::reduce_keys_serial(keys.data(), threads);
                    const Move m = move_decide(a, src, keys[0]);
                    for (int tid = 0; tid < threads; ++tid) move_rowcase(a, src, m, tid, threads);
                }
                for (size_t src = 0; src < (size_t)B; ++src) {
                    if (!a.move[src].ok) continue;                   // (every element returns at once)
                    for (int64_t X = 0; X < rows; ++X) {
                        if (!a.rowcase[src * (size_t)rows + (size_t)X]) continue;
                        for (int v = 0; v < (int)nodes; ++v) update_elem(a, src, X, v);
                    }
                }
            }
            if (between_rounds(B, N, a.parent, a.children, a.steps, a.done, a.status, a.rebuild, fresh.data(), a.depth, &resumes)) break;
        }
        for (size_t src = 0; src < (size_t)B; ++src)
            for (int e = 0; e < (int)root; ++e) edge_length(a, src, e);
    }
};

// ---- balanced subtree pruning and regrafting (pf_bme_spr, pf_bme_spr_device, pf_bme_spr_host, pf_bme_spr_newick_n;
// DESIGN.md section 22).  bme.py::bme_spr is the statement: pair table, candidates, rule and the chain of swaps are
// defined there.  One step, everything from scratch, no host copy in between:
//   number   one thread: entry / exit times and the depth from the root of every node of the rooted tree
//   depth    one thread per (row, node): below edge e by the interval test; beyond its parent end by climbing from
//            parent[e] to the first ancestor whose interval holds the node
//   build    build_elem as it is (M of every row)
//   pairs    T[X][Y], one pairwise sum per entry, by tiles through the workgroup's scratch (pairs_tile_*) or one thread
//            per entry (pairs_elem): the same operands in the same order; 0.0 where X and Y share a leaf
//   eval     one thread per (S row, target edge): it walks its own path from S's attachment node - the next node is the
//            forward neighbour whose directed subtree holds the target, one depth lookup -, adds the terms in path
//            order, and the workgroup's minimum key (dL, S, edge) goes to `spart`
//   move     the minimum of the partial minima; one thread decides (done, capped, or move) and carries the move out as
//            the swaps along the path
// A finished source clears its `rebuild`, so that build_elem returns at once for it too, and keeps depth and M of its
// final topology: the evaluation and the lengths of balanced NNI (eval_q_thread, edge_length) then give q, lengths and
// tree_length exactly as bme.py::Table does.  Args::done stays 0 throughout (it would idle that evaluation); the
// search's own flag is `sdone`.

PF_TAXA_HD inline bool spr_idle(const SprArgs& s, size_t src) { return s.b.status[src] == ST_NONFINITE || s.sdone[src]; }

PF_TAXA_HD inline void number_tree(const SprArgs& s, size_t src) {
    if (spr_idle(s, src)) return;
    const int64_t nodes = nodes_of(s.b.N), root = root_of(s.b.N);
    const int32_t* parent = s.b.parent + (int64_t)src * nodes;
    const int32_t* children = s.b.children + (int64_t)src * nodes * 3;
    int32_t* tin = s.tin + (int64_t)src * nodes;
    int32_t* tout = s.tout + (int64_t)src * nodes;
    int32_t* nd = s.ndepth + (int64_t)src * nodes;
    int32_t t = 0, v = (int32_t)root;
    nd[v] = 0; tin[v] = t++;
    for (int64_t guard = 0; guard < 4 * nodes; ++guard) {            // (every edge is walked twice)
        const int32_t c = children[(int64_t)v * 3];
        if (c >= 0) { nd[c] = nd[v] + 1; tin[c] = t++; v = c; continue; }
        for (;;) {                                                   // v is complete: on to its next sibling, or up
            tout[v] = t - 1;
            if (v == root) return;
            const int32_t p = parent[v];
            const int32_t* pc = children + (int64_t)p * 3;
            const int32_t next = pc[0] == v ? pc[1] : pc[1] == v ? pc[2] : -1;
            if (next >= 0) { nd[next] = nd[p] + 1; tin[next] = t++; v = next; break; }
            v = p;
        }
    }
}

PF_TAXA_HD inline void depth_elem(const SprArgs& s, size_t src, int64_t X, int v) {
    if (spr_idle(s, src)) return;
    const int64_t nodes = nodes_of(s.b.N), root = root_of(s.b.N), rows = rows_of(s.b.N);
    const int32_t* parent = s.b.parent + (int64_t)src * nodes;
    const int32_t* tin = s.tin + (int64_t)src * nodes;
    const int32_t* tout = s.tout + (int64_t)src * nodes;
    const int32_t* nd = s.ndepth + (int64_t)src * nodes;
    const int32_t tv = tin[v];
    const int64_t e = X < root ? X : X - root;
    const bool below = tin[e] <= tv && tv <= tout[e];
    int out = -1;
    if (X < root) {
        if (below) out = nd[v] - nd[e];
    } else if (!below) {
        const int32_t p = parent[e];
        int32_t w = p;
        while (w != root && !(tin[w] <= tv && tv <= tout[w])) w = parent[w];
        out = nd[p] + nd[v] - 2 * nd[w];
    }
    s.b.depth[((int64_t)src * rows + X) * nodes + v] = (int16_t)out;
}

// Do rows X and Y share a leaf?  From the numbering alone: "below e" is the interval of e, "beyond e" its complement.
// Two intervals of a tree are nested or disjoint; a complement meets an interval unless it lies inside the other's
// interval; two complements always meet (the root has three children, so two subtrees never cover the tree).
PF_TAXA_HD inline bool rows_share_leaf(const SprArgs& s, size_t src, int64_t X, int64_t Y) {
    const int64_t nodes = nodes_of(s.b.N), root = root_of(s.b.N);
    const int32_t* tin = s.tin + (int64_t)src * nodes;
    const int32_t* tout = s.tout + (int64_t)src * nodes;
    const int64_t ex = X < root ? X : X - root, ey = Y < root ? Y : Y - root;
    const bool x_in_y = tin[ey] <= tin[ex] && tout[ex] <= tout[ey], y_in_x = tin[ex] <= tin[ey] && tout[ey] <= tout[ex];
    if (X < root && Y < root) return x_in_y || y_in_x;
    if (X < root) return !x_in_y;
    if (Y < root) return !y_in_x;
    return true;
}

// T[X][Y], one thread per entry straight from global memory
PF_TAXA_HD inline void pairs_elem(const SprArgs& s, size_t src, int64_t X, int64_t Y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (spr_idle(s, src)) return;
    const int64_t rows = rows_of(s.b.N);
    double v = 0.0;
    if (!rows_share_leaf(s, src, X, Y)) {
        const double* m = M_row(s.b, src, X);
        const int16_t* dy = depth_row(s.b, src, Y);
        v = pfnj::pairwise_sum([&](int j) { return weight(dy[j]) * m[j]; }, s.b.N);
    }
    s.T[((int64_t)src * rows + X) * rows + Y] = v;
}

// pfnj::pairwise_sum's walk (a second statement of the same split: see the note there) as a sequence of events, so
// that a workgroup can take it together: 1 = the leaf (lo, cnt),
// cnt <= 128, whose pfnj::leaf_sum is pushed; 2 = the two values on top are replaced by their sum (left + right); 0 =
// the end, the sum is the one value left.  The events depend on n alone.
struct SumWalk {
    int w_lo[pfnj::WALK_DEPTH], w_n[pfnj::WALK_DEPTH], sp;
    PF_TAXA_HD void start(int n) { w_lo[0] = 0; w_n[0] = n; sp = 1; }
    PF_TAXA_HD int next(int* lo, int* cnt) {
        while (sp > 0) {
            --sp;
            const int l = w_lo[sp], c = w_n[sp];
            if (c == 0) return 2;
            if (c <= 128) { *lo = l; *cnt = c; return 1; }
            int n2 = c / 2;
            n2 -= n2 % 8;
            w_lo[sp] = 0; w_n[sp] = 0; ++sp;
            w_lo[sp] = l + n2; w_n[sp] = c - n2; ++sp;
            w_lo[sp] = l; w_n[sp] = n2; ++sp;
        }
        return 0;
    }
};

// T by tiles: a workgroup of PAIR_TILE^2 threads owns the entries (X, Y) of tile (tx, ty), thread tid the entry
// (tx * PAIR_TILE + tid / PAIR_TILE, ty * PAIR_TILE + tid % PAIR_TILE).  It takes SumWalk's events together: for a leaf,
// every thread first stages its share of M[X][lo .. lo + cnt) and of w_Y(lo .. lo + cnt) (from depth, once per (Y, j)
// instead of once per entry) into `lm` / `lw` [PAIR_TILE][PAIR_STRIDE]; after a barrier every thread forms
// pfnj::leaf_sum of its entry from them and pushes it.  The operands and their order are pairs_elem's.  PAIR_STRIDE =
// 129 doubles: the PAIR_TILE rows a wave reads at one j lie 2 banks apart.
constexpr int PAIR_TILE = 16, PAIR_STRIDE = 129;
struct PairThread {
    double val[pfnj::WALK_DEPTH];
    int vp;
    bool active;            // inside the table and without a common leaf
};
PF_TAXA_HD inline void pairs_tile_begin(const SprArgs& s, size_t src, int tx, int ty, int tid, PairThread& t) {
    const int64_t rows = rows_of(s.b.N), X = (int64_t)tx * PAIR_TILE + tid / PAIR_TILE, Y = (int64_t)ty * PAIR_TILE + tid % PAIR_TILE;
    t.vp = 0;
    t.active = X < rows && Y < rows && !rows_share_leaf(s, src, X, Y);
}
PF_TAXA_HD inline void pairs_tile_stage(const SprArgs& s, size_t src, int tx, int ty, int lo, int cnt, int tid, int threads, double* lm,
                                        double* lw) {
    const int64_t rows = rows_of(s.b.N);
    for (int i = tid; i < 2 * PAIR_TILE * cnt; i += threads) {
        const int r = i / cnt % PAIR_TILE, j = i % cnt;
        if (i < PAIR_TILE * cnt) {
            const int64_t X = (int64_t)tx * PAIR_TILE + r;
            lm[r * PAIR_STRIDE + j] = X < rows ? M_row(s.b, src, X)[lo + j] : 0.0;
        } else {
            const int64_t Y = (int64_t)ty * PAIR_TILE + r;
            lw[r * PAIR_STRIDE + j] = Y < rows ? weight(depth_row(s.b, src, Y)[lo + j]) : 0.0;
        }
    }
}
PF_TAXA_HD inline void pairs_tile_leaf(int cnt, int tid, const double* lm, const double* lw, PairThread& t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!t.active) return;
    const double* m = lm + (tid / PAIR_TILE) * PAIR_STRIDE;
    const double* w = lw + (tid % PAIR_TILE) * PAIR_STRIDE;
    t.val[t.vp++] = pfnj::leaf_sum([&](int j) { return w[j] * m[j]; }, 0, cnt);
}
PF_TAXA_HD inline void pairs_tile_add(PairThread& t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!t.active) return;
    const double right = t.val[--t.vp], left = t.val[--t.vp];
    t.val[t.vp++] = left + right;
}
PF_TAXA_HD inline void pairs_tile_end(const SprArgs& s, size_t src, int tx, int ty, int tid, const PairThread& t) {
    const int64_t rows = rows_of(s.b.N), X = (int64_t)tx * PAIR_TILE + tid / PAIR_TILE, Y = (int64_t)ty * PAIR_TILE + tid % PAIR_TILE;
    if (X < rows && Y < rows) s.T[((int64_t)src * rows + X) * rows + Y] = t.active ? t.val[0] : 0.0;
}

// the row of the directed subtree through neighbour v of node u, away from u
PF_TAXA_HD inline int64_t row_through(const int32_t* parent, int64_t root, int32_t v, int32_t u) { return parent[v] == u ? (int64_t)v : root + u; }
// the two neighbours of internal node u besides prev
PF_TAXA_HD inline void forward_of(const int32_t* parent, const int32_t* children, int64_t root, int32_t u, int32_t prev, int32_t* f) {
    int n = 0;
    f[0] = f[1] = -1;
    for (int i = 0; i < 3; ++i) {
        const int32_t c = children[(int64_t)u * 3 + i];
        if (c >= 0 && c != prev && n < 2) f[n++] = c;
    }
    if (u != root && parent[u] != prev && n < 2) f[n++] = parent[u];
}

// The candidate (S row, target edge g): its key, or none when S cannot be regrafted there (g inside S, or on S's
// attachment node, or that node a leaf).  `path`, when not NULL, receives u_1 .. u_i, t and `path_len` their number.
PF_TAXA_HD inline Key spr_candidate(const SprArgs& s, size_t src, int64_t S, int32_t g, int32_t* path, int32_t* path_len) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int N = s.b.N;
    const int64_t nodes = nodes_of(N), root = root_of(N), rows = rows_of(N);
    const int32_t* parent = s.b.parent + (int64_t)src * nodes;
    const int32_t* children = s.b.children + (int64_t)src * nodes * 3;
    const double* T = s.T + (int64_t)src * rows * rows;
    const int32_t e = (int32_t)(S < root ? S : S - root);
    const int32_t snode = S < root ? e : parent[e], a = S < root ? parent[e] : e;
    const int32_t pg = parent[g];
    if (a < N || g == a || pg == a) return key_none();
    const int16_t* ds = depth_row(s.b, src, S);
    if (ds[g] >= 0 || ds[pg] >= 0) return key_none();
    int32_t f[2];
    forward_of(parent, children, root, a, snode, f);
    if (f[1] < 0) return key_none();
    int32_t u = depth_row(s.b, src, row_through(parent, root, f[0], a))[g] >= 0 ? f[0] : f[1];
    const int64_t R = row_through(parent, root, u == f[0] ? f[1] : f[0], a);
    double drs = T[R * rows + S], acc = 0.0;
    int32_t prev = a;
    for (int i = 1; i < (int)nodes; ++i) {
        forward_of(parent, children, root, u, prev, f);
        if (f[1] < 0) break;                                        // (a leaf on the path: never with a valid tree)
        const bool last = u == g || u == pg;
        const int32_t next = last ? (u == g ? pg : g) : depth_row(s.b, src, row_through(parent, root, f[0], u))[g] >= 0 ? f[0] : f[1];
        const int64_t X = row_through(parent, root, f[0] == next ? f[1] : f[0], u), F = row_through(parent, root, next, u),
                      Bk = row_through(parent, root, prev, u);
        const double scaled = weight(i) * (T[R * rows + X] - T[S * rows + X]);
        const double drx = T[Bk * rows + X] + scaled;
        const double term = 0.25 * ((drx + T[S * rows + F]) - (drs + T[X * rows + F]));
        acc = acc + term;
        if (path) path[i - 1] = u;
        if (last) {
            if (path) { path[i] = next; *path_len = i + 1; }
            return Key{acc, (int32_t)S, g};                          // (value, S row, target edge)
        }
        const double half = 0.5 * T[X * rows + S];
        drs = 0.5 * drs + half;
        prev = u; u = next;
    }
    return key_none();                                              // never with a valid tree
}

// Thread `tid` of the evaluation's workgroup (S, wg): the target edges wg * epg + tid, + threads, ... below (wg + 1) * epg
PF_TAXA_HD inline Key spr_eval_thread(const SprArgs& s, size_t src, int64_t S, int wg, int tid, int threads) {
    Key best = key_none();
    if (spr_idle(s, src)) return best;
    const int64_t root = root_of(s.b.N);
    for (int64_t g = (int64_t)wg * s.epg + tid; g < ((int64_t)wg + 1) * s.epg && g < root; g += threads) {
        const Key k = spr_candidate(s, src, S, (int32_t)g, nullptr, nullptr);
        if (key_less(k, best)) best = k;
    }
    return best;
}

PF_TAXA_HD inline Key spr_move_thread_key(const SprArgs& s, size_t src, int tid, int threads) {
    Key best = key_none();
    if (spr_idle(s, src)) return best;
    const Key* part = s.spart + src * (size_t)s.spart_cap;
    for (int g = tid; g < s.spart_cap; g += threads)
        if (key_less(part[g], best)) best = part[g];
    return best;
}

// One thread: no qualifying candidate - the source is done; the cap reached - done and capped; else the move, as
// bme.py::spr_move's swaps along the path.
PF_TAXA_HD inline void spr_decide(const SprArgs& s, size_t src, Key best) {
    if (spr_idle(s, src)) return;
    const int N = s.b.N;
    const int64_t nodes = nodes_of(N), root = root_of(N), rows = rows_of(N);
    if (!(best.v < THRESHOLD)) { s.sdone[src] = 1; s.b.rebuild[src] = 0; return; }
    if (s.b.steps[src] >= s.cap) { s.b.status[src] = ST_CAPPED; s.sdone[src] = 1; s.b.rebuild[src] = 0; return; }
    int32_t* path = s.path + (int64_t)src * nodes;
    int32_t len = 0;
    if (best.a < 0 || best.a >= rows || best.b < 0 || best.b >= root ||               // (S row, target edge)
        !(spr_candidate(s, src, best.a, best.b, path, &len).v < THRESHOLD)) {            // never with finite input
        s.b.status[src] = ST_NONFINITE; s.b.rebuild[src] = 0; return;
    }
    int32_t* parent = s.b.parent + (int64_t)src * nodes;
    int32_t* children = s.b.children + (int64_t)src * nodes * 3;
    const bool below = best.a < root;
    const int32_t e = (int32_t)(below ? best.a : best.a - root);
    for (int32_t j = 0; j + 1 < len; ++j) {
        const int32_t u = path[j], next = path[j + 1], v = below ? parent[e] : e;
        if (parent[u] == v) {               // down: S stands beside edge u as s or as A, X_j is a child of u
            const Quartet t = quartet_of(parent, children, root, u);
            const bool next_first = t.c1 == next;
            const bool take_next = !(below && t.s == e);
            const bool first = take_next == next_first;
            swap_blocks(parent, children, root, u, t.p, t.s, first ? t.c1 : t.c2, first ? t.c2 : t.c1);
        } else {                            // up: S is child e of v, X_j stands beside edge v as s or as A
            const Quartet t = quartet_of(parent, children, root, v);
            const bool e_first = t.c1 == e;
            const bool take_e = next != t.s;
            const bool first = take_e == e_first;
            swap_blocks(parent, children, root, v, t.p, t.s, first ? t.c1 : t.c2, first ? t.c2 : t.c1);
        }
    }
    s.b.steps[src] += 1;
}

// an array of the state under its name, as a driver reads it
template <class T>
struct ArrayView {
    T* p = nullptr;
    T& operator[](size_t i) const { return p[i]; }
    T* data() const { return p; }
};

// The serial run of the search's bodies in the order the launches of pf_bme.hip.h give them.
struct SprSerial : SerialBase {
    bool tiled = false;       // T by pairs_tile_* instead of pairs_elem: the same bits
    // what tests/native/pf_spr_main.cpp compares and writes step by step
    ArrayView<int32_t> parent, children, steps;
    ArrayView<int16_t> depth;
    ArrayView<double> T;

    bool setup(const float* preds, const int32_t* start_slots, int B_, int N_, int epg, int64_t cap = -1) {
        B = B_; N = N_;
        s = spr_args_of(preds, N, 1, epg, cap < 0 ? step_cap(N) : cap);        // (finish: one workgroup, its minimum unused)
        spr_state_arrays(mem, s, (size_t)B);
        parent.p = a.parent; children.p = a.children; steps.p = a.steps; depth.p = a.depth; T.p = s.T;
        return start_trees(start_slots);
    }

    // number, depth, build and pairs of one step (the table the evaluation reads)
    void table(bool rows_at_once) {
        const int64_t rows = rows_of(N), nodes = nodes_of(N);
        for (size_t src = 0; src < (size_t)B; ++src) {
            number_tree(s, src);
            for (int64_t X = 0; X < rows; ++X)
                for (int v = 0; v < (int)nodes; ++v) depth_elem(s, src, X, v);
            for (int64_t X = 0; X < rows; ++X) {
                if (rows_at_once) { build_row(s.b, src, X); continue; }
                for (int j = 0; j < N; ++j) build_elem(s.b, src, X, j);
            }
            if (tiled) pairs_tiled(src);
            else
                for (int64_t X = 0; X < rows; ++X)
                    for (int64_t Y = 0; Y < rows; ++Y) pairs_elem(s, src, X, Y);
        }
    }

    // the tiled bodies in the order of k_bme_pairs: a tile without an active entry writes its zeros and leaves
    void pairs_tiled(size_t src) {
        constexpr int threads = PAIR_TILE * PAIR_TILE;
        const int tiles = (int)((rows_of(N) + PAIR_TILE - 1) / PAIR_TILE);
        std::vector<PairThread> t((size_t)threads);
        std::vector<double> lm((size_t)PAIR_TILE * PAIR_STRIDE), lw((size_t)PAIR_TILE * PAIR_STRIDE);
        if (spr_idle(s, src)) return;
        for (int tx = 0; tx < tiles; ++tx)
            for (int ty = 0; ty < tiles; ++ty) {
                bool any = false;
                for (int tid = 0; tid < threads; ++tid) { pairs_tile_begin(s, src, tx, ty, tid, t[(size_t)tid]); any |= t[(size_t)tid].active; }
                SumWalk walk;
                walk.start(N);
                int lo = 0, cnt = 0;
                for (int ev = any ? walk.next(&lo, &cnt) : 0; ev; ev = walk.next(&lo, &cnt)) {
                    if (ev == 2) { for (int tid = 0; tid < threads; ++tid) pairs_tile_add(t[(size_t)tid]); continue; }
                    for (int tid = 0; tid < threads; ++tid) pairs_tile_stage(s, src, tx, ty, lo, cnt, tid, threads, lm.data(), lw.data());
                    for (int tid = 0; tid < threads; ++tid) pairs_tile_leaf(cnt, tid, lm.data(), lw.data(), t[(size_t)tid]);
                }
                for (int tid = 0; tid < threads; ++tid) pairs_tile_end(s, src, tx, ty, tid, t[(size_t)tid]);
            }
    }

    void evaluate_and_move(int threads) {
        const int64_t rows = rows_of(N);
        const int G = eval_groups(N, s.epg);
        std::vector<Key> keys((size_t)threads);
        for (size_t src = 0; src < (size_t)B; ++src) {
            for (int64_t S = 0; S < rows; ++S)
                for (int wg = 0; wg < G; ++wg) {
                    for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = spr_eval_thread(s, src, S, wg, tid, threads);
                    pfnj::reduce_keys_serial(keys.data(), threads);
                    s.spart[src * (size_t)s.spart_cap + (size_t)(S * G + wg)] = keys[0];
                }
            for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = spr_move_thread_key(s, src, tid, threads);
            pfnj::reduce_keys_serial(keys.data(), threads);
            spr_decide(s, src, keys[0]);
        }
    }

    bool finished() const {
        for (size_t src = 0; src < (size_t)B; ++src)
            if (!spr_idle(s, src)) return false;
        return true;
    }

    // q and the lengths of the final topology (one workgroup of `threads` threads over all edges)
    void finish(int threads) {
        const int epg = (int)root_of(N);
        std::vector<double> lq((size_t)epg * 6);
        for (size_t src = 0; src < (size_t)B; ++src) {
            for (int tid = 0; tid < threads; ++tid) eval_q_thread(s.b, src, 0, epg, tid, threads, lq.data());
            for (int e = 0; e < epg; ++e) edge_length(s.b, src, e);
        }
    }

    void run(int threads, int init_groups, bool rows_at_once = false) {
        init(threads, init_groups);
        while (!finished())
            for (int step = 0; step < ROUND_STEPS; ++step) { table(rows_at_once); evaluate_and_move(threads); }
        finish(threads);
    }
};

}  // namespace pfbme
