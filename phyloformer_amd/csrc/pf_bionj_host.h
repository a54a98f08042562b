// BIONJ on the device (pf_bionj_joins, pf_bionj_joins_device): the bodies of the kernels of
// pf_bionj.hip.h as functions of (source, workgroup, thread).  Plain C++, no HIP: tests/native/pf_bionj_main.cpp runs
// them on the CPU thread by thread under AddressSanitizer / UBSan, pf_bionj.hip.h compiles them for the device too
// (PF_TAXA_HD), and run_serial - the same bodies with one workgroup of one thread - is pf_bionj_joins_host.
// phyloformer_amd/bionj.py::bionj_joins is the statement of the algorithm: every float64 operation here happens with
// the same operands in the same order as there, so the tables are bit-identical.
//
// Per source: pf_nj_host.h's state (d [N][N], the row sums r [N], the two copies of the list of active rows, the
// partial minima of q) and beside it the variances v [N][N], the partial minima of the scan index, and label [N], the
// smallest sequence of the cluster that lives in a row.  The join table is pf_nj_host.h's.
//
// A join is two minima of total orders.  q* is the minimum of (q, x, y) over the positions y < x - only its value is
// used -, and the pair is the minimum of (x, y) over the pairs with q <= q* + EPS, q re-evaluated by the same
// operations and hence with the same bits: the first pair of the scan (1,0), (2,0), (2,1), (3,0), ... inside the
// window, however the pairs are split among threads and workgroups.  The joined cluster takes the row of the later
// position x; position y leaves the list.  Finite input only: a source with a NaN or an infinity is flagged by
// init_elems and every later body returns at once for it (its table is unspecified).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pf_nj_host.h"

namespace pfbionj {

using pfnj::Key;
using pfnj::key_less;
using pfnj::key_none;
using pfnj::table_len;

constexpr double EPS = 1e-9;           // bionj.py::EPS: the window of the pick

struct Args {
    pfnj::Args nj;          // preds, d, r, part (the minima of q), active, slots, lengths, flag, N, part_cap, PN
    double* v;              // [B][N][N]
    Key* part_at;           // [B][part_cap]: the first pair inside the window of every workgroup of k_bionj_pick
    int32_t* label;         // [B][N]
};

// Thread `tid` of workgroup `wg` of `G`: the elements e = (wg * threads + tid), + G * threads, ... of d and v (v = d,
// formed as pfnj::init_elems forms d), the first list of active rows and the labels.
PF_TAXA_HD inline void init_elems(const Args& a, size_t src, int wg, int G, int tid, int threads) {
    const int64_t N = a.nj.N, NN = N * N;
    const float* preds = a.nj.preds + src * (size_t)a.nj.PN;
    double* d = a.nj.d + src * (size_t)NN;
    double* v = a.v + src * (size_t)NN;
    int32_t* act = a.nj.active + src * 2 * (size_t)N;
    int32_t* label = a.label + src * (size_t)N;
    bool bad = false;
    for (int64_t e = (int64_t)wg * threads + tid; e < NN; e += (int64_t)G * threads) {
        const int64_t i = e / N, j = e % N;
        if (e < N) { act[e] = (int32_t)e; label[e] = (int32_t)e; }
        if (i == j) { d[e] = 0.0; v[e] = 0.0; continue; }
        const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
        const float x = preds[lo * N - lo * (lo + 1) / 2 + (hi - lo - 1)];
        bad |= !(x - x == 0.0f);                               // NaN or infinite
        d[e] = (double)(x + 0.0f);
        v[e] = (double)(x + 0.0f);
    }
    if (bad) a.nj.flag[src] = 1;
}

// q of positions y < x of join t: ((m - 2) d_xy - r[x]) - r[y], two roundings after the product, no FMA; read at
// d[row x][row y]
struct Criterion {
    const int32_t* act;
    const double* d;
    const double* r;
    size_t N;
    double mm2;
    PF_TAXA_HD inline double operator()(int x, int y) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double prod = mm2 * d[(size_t)act[x] * N + (size_t)act[y]];
        return (prod - r[x]) - r[y];
    }
};
PF_TAXA_HD inline Criterion criterion_of(const Args& a, int m, int t, size_t src) {
    const size_t N = (size_t)a.nj.N;
    return Criterion{pfnj::active_of(a.nj, src, t), a.nj.d + src * N * N, a.nj.r + src * N, N, (double)(m - 2)};
}

// Thread `tid` of workgroup `wg` of `G` on the pairs of join t: positions x = wg, wg + G, ... and y = tid,
// tid + threads, ... < x.  The minimum key (q, x, y).
PF_TAXA_HD inline Key qmin_thread(const Args& a, int m, int t, size_t src, int wg, int G, int tid, int threads) {
    Key best = key_none();
    if (a.nj.flag[src]) return best;
    const Criterion q = criterion_of(a, m, t, src);
    for (int x = wg; x < m; x += G)
        for (int y = tid; y < x; y += threads) {
            const Key k{q(x, y), x, y};
            if (key_less(k, best)) best = k;
        }
    return best;
}

// The same thread's pairs once more, q* known: the first pair of the scan with q <= q* + EPS, as the key (0, x, y) -
// ordered by (x, y), which is the order of the scan.
PF_TAXA_HD inline Key pick_thread(const Args& a, int m, int t, size_t src, double qstar, int wg, int G, int tid, int threads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    Key best = key_none();
    if (a.nj.flag[src]) return best;
    const Criterion q = criterion_of(a, m, t, src);
    const double bound = qstar + EPS;
    for (int x = wg; x < m; x += G)
        for (int y = tid; y < x; y += threads) {
            if (!(q(x, y) <= bound)) continue;
            const Key k{0.0, x, y};
            if (key_less(k, best)) best = k;
        }
    return best;
}

// thread `tid` of a workgroup: the minimum of the partial keys tid, tid + threads, ... of the G in `part`
PF_TAXA_HD inline Key part_thread_key(const Args& a, const Key* part, size_t src, int G, int tid, int threads) {
    Key best = key_none();
    if (a.nj.flag[src]) return best;
    part += src * (size_t)a.nj.part_cap;
    for (int g = tid; g < G; g += threads)
        if (key_less(part[g], best)) best = part[g];
    return best;
}

// what one thread works out of the pick and all threads of the join read (through LDS on the device)
struct Join { int32_t ry, rx, pos_y, ok; double ly, lx, lam, om, c; };

// Join t from the first pair inside the window: positions y < x, their rows, the branch lengths, lambda; writes the
// table and the new cluster's label.  One thread: lambda's sum is pairwise_sum over the active positions in order.
// ok = 0: a flagged source, or - never with finite input - a pair outside the matrix (the source is flagged then).
PF_TAXA_HD inline Join join_record(const Args& a, int m, int t, size_t src, Key best) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    Join j{0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.nj.flag[src]) return j;
    if (best.b < 0 || best.a >= m || best.b >= best.a) { a.nj.flag[src] = 1; return j; }
    const size_t N = (size_t)a.nj.N;
    const int32_t* act = pfnj::active_of(a.nj, src, t);
    const double* r = a.nj.r + src * N;
    const int px = best.a, py = best.b;
    j.rx = act[px]; j.ry = act[py]; j.pos_y = py; j.ok = 1;
    const double dxy = a.nj.d[src * N * N + (size_t)j.rx * N + (size_t)j.ry];
    j.ly = 0.5 * dxy + (r[py] - r[px]) / (double)(2 * ((int64_t)m - 2));
    j.lx = dxy - j.ly;
    const double* vy = a.v + src * N * N + (size_t)j.ry * N;
    const double* vx = a.v + src * N * N + (size_t)j.rx * N;
    const double vxy = vx[j.ry];
    double lam = 0.5;
    if (vxy != 0.0) {
        const double s = pfnj::pairwise_sum([&](int k) { return k == py || k == px ? 0.0 : vx[act[k]] - vy[act[k]]; }, m);
        lam = 0.5 + s / ((double)(2 * ((int64_t)m - 2)) * vxy);
        lam = !(lam >= 0.0) ? 0.0 : (lam > 1.0 ? 1.0 : lam);
    }
    j.lam = lam;
    j.om = 1.0 - lam;
    j.c = (lam * j.om) * vxy;
    int32_t* label = a.label + src * N;
    const int32_t by = label[j.ry], bx = label[j.rx];
    const size_t at = src * (size_t)table_len(a.nj.N) + 2 * (size_t)t;
    a.nj.slots[at] = by < bx ? by : bx;  a.nj.slots[at + 1] = by < bx ? bx : by;
    a.nj.lengths[at] = by < bx ? j.ly : j.lx;  a.nj.lengths[at + 1] = by < bx ? j.lx : j.ly;
    label[j.rx] = by < bx ? by : bx;
    return j;
}

// Thread `tid` of the join's workgroup after join_record: row and column rx of d and v become the new cluster's for
// all k < N, zero at [rx][rx], and position pos_y leaves the list of active rows.  Thread k reads [ry][k] and [rx][k]
// and writes [rx][k] and [k][rx]; k = rx only writes the zeros (nobody reads [ry][rx], which thread ry writes).
PF_TAXA_HD inline void join_update(const Args& a, int m, int t, size_t src, const Join& j, int tid, int threads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!j.ok) return;
    const size_t N = (size_t)a.nj.N, ry = (size_t)j.ry, rx = (size_t)j.rx;
    double* d = a.nj.d + src * N * N;
    double* v = a.v + src * N * N;
    for (size_t k = (size_t)tid; k < N; k += (size_t)threads) {
        if (k == rx) { d[rx * N + rx] = 0.0; v[rx * N + rx] = 0.0; continue; }
        const double dy = d[ry * N + k] - j.ly, dx = d[rx * N + k] - j.lx;
        const double dn = j.lam * dy + j.om * dx;
        const double vn = (j.lam * v[ry * N + k] + j.om * v[rx * N + k]) - j.c;
        d[rx * N + k] = dn;
        d[k * N + rx] = dn;
        v[rx * N + k] = vn;
        v[k * N + rx] = vn;
    }
    const int32_t* act = pfnj::active_of(a.nj, src, t);
    int32_t* next = a.nj.active + (src * 2 + (size_t)((t + 1) & 1)) * N;
    for (int p = tid; p < m - 1; p += threads) next[p] = act[p + (p >= j.pos_y ? 1 : 0)];
}

// after the last join: pf_nj_host.h's trifurcation of the three remaining rows in active order, written in ascending
// order of their labels
PF_TAXA_HD inline void final_record(const Args& a, size_t src) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (a.nj.flag[src]) return;
    const size_t N = (size_t)a.nj.N;
    const int32_t* act = pfnj::active_of(a.nj, src, a.nj.N - 3);
    const int32_t* label = a.label + src * N;
    const double* d = a.nj.d + src * N * N;
    const size_t i = (size_t)act[0], j = (size_t)act[1], k = (size_t)act[2];
    int32_t s[3] = {label[i], label[j], label[k]};
    double l[3] = {0.5 * ((d[i * N + j] + d[i * N + k]) - d[j * N + k]), 0.5 * ((d[i * N + j] + d[j * N + k]) - d[i * N + k]),
                   0.5 * ((d[i * N + k] + d[j * N + k]) - d[i * N + j])};
    for (int p = 0; p < 2; ++p)                                  // three elements: two passes of neighbours
        for (int e = 0; e < 2 - p; ++e)
            if (s[e + 1] < s[e]) {
                const int32_t ts = s[e]; s[e] = s[e + 1]; s[e + 1] = ts;
                const double tl = l[e]; l[e] = l[e + 1]; l[e + 1] = tl;
            }
    const size_t at = src * (size_t)table_len(a.nj.N) + 2 * (N - 3);
    for (int e = 0; e < 3; ++e) { a.nj.slots[at + (size_t)e] = s[e]; a.nj.lengths[at + (size_t)e] = l[e]; }
}

// ---- the arrays of a state, listed once (pf_spans.h has the visitors); the staging is pfnj::staging_arrays ----------
inline Args args_of(const float* preds, int N, int part_cap, int32_t* slots, double* lengths, uint8_t* flag) {
    Args a{};
    a.nj = pfnj::args_of(preds, N, part_cap, slots, lengths, flag);
    return a;
}

template <class V>
inline void state_arrays(V& v, Args& a, size_t B) {
    const size_t n = (size_t)a.nj.N;
    pfnj::state_arrays(v, a.nj, B);
    v(a.v, B * n * n);
    v(a.part_at, B * (size_t)a.nj.part_cap);
    v(a.label, B * n);
}

// bytes of one source's state on the device
inline size_t state_bytes(int N) {
    Args a = args_of(nullptr, N, pfnj::Q_GROUPS, nullptr, nullptr, nullptr);
    return pfspan::measure([&](auto& v) { state_arrays(v, a, 1); });
}

// the state of B sources carved from `ws` (8-byte aligned, B * state_bytes(N) bytes)
inline Args carve(char* ws, const float* preds, int B, int N, int32_t* slots, double* lengths, uint8_t* flag) {
    Args a = args_of(preds, N, pfnj::Q_GROUPS, slots, lengths, flag);
    pfspan::carve(ws, [&](auto& v) { state_arrays(v, a, (size_t)B); });
    return a;
}

// The whole join sequence of B sources on the CPU: every body as its one workgroup of one thread.  flag [B] is zeroed
// here; a flagged source's table is left as it was.
inline void run_serial(const float* preds, int B, int N, int32_t* slots, double* lengths, uint8_t* flag) {
    Args a = args_of(preds, N, 1, slots, lengths, flag);
    pfspan::Allocate mem;
    state_arrays(mem, a, (size_t)B);
    for (size_t src = 0; src < (size_t)B; ++src) {
        flag[src] = 0;
        init_elems(a, src, 0, 1, 0, 1);
        for (int t = 0; t < N - 3; ++t) {
            const int m = N - t;
            for (int row = 0; row < m; ++row) pfnj::row_sum(a.nj, m, t, src, row);
            a.nj.part[src] = qmin_thread(a, m, t, src, 0, 1, 0, 1);
            a.part_at[src] = pick_thread(a, m, t, src, a.nj.part[src].v, 0, 1, 0, 1);
            const Join j = join_record(a, m, t, src, a.part_at[src]);
            join_update(a, m, t, src, j, 0, 1);
        }
        final_record(a, src);
    }
}

}  // namespace pfbionj
