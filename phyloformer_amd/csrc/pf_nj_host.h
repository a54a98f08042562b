// Neighbour joining on the device (pf_nj_joins, pf_nj_joins_device): the bodies of the kernels of
// pf_nj.hip.h as functions of (source, workgroup, thread).  Plain C++, no HIP: tests/native/pf_nj_main.cpp runs them on
// the CPU thread by thread under AddressSanitizer / UBSan; pf_nj.hip.h compiles them for the device too (PF_TAXA_HD).
// phyloformer_amd/nj.py::nj_joins is the statement of the algorithm and pf_hostio.cpp::nj_core its native twin: every
// float64 operation here happens with the same operands in the same order as there, so the joins are bit-identical.
//
// Per source: the symmetric double d [N][N] (built as pf_hostio.cpp::pair_at does, zero diagonal), the row sums
// r [N], the list of active slots (two copies: join t reads copy t & 1 and writes the other, so that erasing a
// position is not an in-place shift), the partial minima of Q, and the join table:
//   slots   int32  [2 (N - 3) + 3]   a, b of every join (slot a < slot b; the new cluster takes slot a), then i, j, k
//   lengths double [2 (N - 3) + 3]   la, lb of every join, then li, lj, lk of the trifurcation
// Join t has m = N - t active slots.  Finite input only: a source with a NaN or an infinity is flagged by init_elems
// and every later body returns at once for it (its table is unspecified).  With finite float32 input nothing here
// overflows or produces a NaN, so the minimum of Q is the minimum of a total order on (value, a, b): any reduction order
// gives np.argmin's first minimum in row-major order.
//
// Key and its minimum serve balanced NNI and balanced SPR too (pf_bme_host.h).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pf_spans.h"
#include "pf_taxa_host.h"

namespace pfnj {

constexpr int Q_GROUPS = 256;          // the most workgroups of the minimum of Q: the partial minima of a source

// A value and where it stands; ordered by (v, a, b).  Here an element of Q at (a, b); pf_bme_host.h says at each use
// what a and b are there.
struct Key { double v; int32_t a, b; };

PF_TAXA_HD inline Key key_none() { return Key{INFINITY, INT32_MAX, INT32_MAX}; }
PF_TAXA_HD inline bool key_less(const Key& x, const Key& y) {
    return x.v < y.v || (x.v == y.v && (x.a < y.a || (x.a == y.a && x.b < y.b)));
}

// entries of a source's join table
PF_TAXA_HD inline int64_t table_len(int N) { return 2 * ((int64_t)N - 3) + 3; }

struct Args {
    const float* preds;     // [B][P_N]
    double* d;              // [B][N][N]
    double* r;              // [B][N]
    Key* part;              // [B][part_cap]: the minimum of every workgroup of k_nj_qmin
    int32_t* active;        // [B][2][N]
    int32_t* slots;         // [B][table_len]
    double* lengths;        // [B][table_len]
    uint8_t* flag;          // [B]: non-finite input (zeroed before init_elems)
    int N, part_cap;
    int64_t PN;
};

PF_TAXA_HD inline const int32_t* active_of(const Args& a, size_t src, int t) { return a.active + (src * 2 + (size_t)(t & 1)) * (size_t)a.N; }

// Thread `tid` of workgroup `wg` of `G`: the elements e = (wg * threads + tid), + G * threads, ... of d, and the first
// list of active slots.  (pfbme::init_elems forms d by the same statements; one shared body compiles to other device
// code for k_nj_init and k_bme_init, so there are two.)
PF_TAXA_HD inline void init_elems(const Args& a, size_t src, int wg, int G, int tid, int threads) {
    const int64_t N = a.N, NN = N * N;
    const float* preds = a.preds + src * (size_t)a.PN;
    double* d = a.d + src * (size_t)NN;
    int32_t* act = a.active + src * 2 * (size_t)N;
    bool bad = false;
    for (int64_t e = (int64_t)wg * threads + tid; e < NN; e += (int64_t)G * threads) {
        const int64_t i = e / N, j = e % N;
        if (e < N) act[e] = (int32_t)e;
        if (i == j) { d[e] = 0.0; continue; }
        const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
        const float x = preds[lo * N - lo * (lo + 1) / 2 + (hi - lo - 1)];
        bad |= !(x - x == 0.0f);                               // NaN or infinite
        d[e] = (double)(x + 0.0f);
    }
    if (bad) a.flag[src] = 1;
}

// numpy's add.reduce of at(lo) .. at(lo + n - 1), n <= 128 (DOUBLE_pairwise_sum's leaves)
template <class At>
PF_TAXA_HD inline double leaf_sum(At&& at, int lo, int n) {
    if (n < 8) {
        double res = -0.0;
        for (int i = 0; i < n; ++i) res += at(lo + i);
        return res;
    }
    double r0 = at(lo), r1 = at(lo + 1), r2 = at(lo + 2), r3 = at(lo + 3), r4 = at(lo + 4), r5 = at(lo + 5), r6 = at(lo + 6),
           r7 = at(lo + 7);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += at(lo + i);     r1 += at(lo + i + 1); r2 += at(lo + i + 2); r3 += at(lo + i + 3);
        r4 += at(lo + i + 4); r5 += at(lo + i + 5); r6 += at(lo + i + 6); r7 += at(lo + i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += at(lo + i);
    return res;
}

// levels of the split of n <= 65536 elements down to leaves of <= 128: at most 10; the work stack holds two entries
// per level and one more
constexpr int WALK_DEPTH = 32;

// numpy's pairwise sum of at(0) .. at(n - 1): more than 128 elements split at n / 2 - (n / 2) % 8, recursively.  The
// recursion is walked with an explicit stack (left before right, then their sum): the tree depends on n only.
// (pf_bme_host.h::SumWalk states the same split as a sequence of events; the two are kept apart because the device
// code of this one changes when it is written on top of the other.)
template <class At>
PF_TAXA_HD inline double pairwise_sum(At&& at, int n) {
    if (n <= 128) return leaf_sum(at, 0, n);
    int w_lo[WALK_DEPTH], w_n[WALK_DEPTH];         // w_n = 0: add the two values on top
    double val[WALK_DEPTH];
    int sp = 0, vp = 0;
    w_lo[sp] = 0; w_n[sp] = n; ++sp;
    while (sp > 0) {
        --sp;
        const int lo = w_lo[sp], cnt = w_n[sp];
        if (cnt == 0) {
            const double right = val[--vp], left = val[--vp];
            val[vp++] = left + right;
        } else if (cnt <= 128) {
            val[vp++] = leaf_sum(at, lo, cnt);
        } else {
            int n2 = cnt / 2;
            n2 -= n2 % 8;
            w_lo[sp] = 0; w_n[sp] = 0; ++sp;
            w_lo[sp] = lo + n2; w_n[sp] = cnt - n2; ++sp;
            w_lo[sp] = lo; w_n[sp] = n2; ++sp;
        }
    }
    return val[0];
}

// r[row] of join t: the sum of row `row` of the active sub-matrix in `active` order, diagonal included, read through
// the symmetric element so that neighbouring rows read neighbouring addresses
PF_TAXA_HD inline void row_sum(const Args& a, int m, int t, size_t src, int row) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (a.flag[src]) return;
    const size_t N = (size_t)a.N;
    const int32_t* act = active_of(a, src, t);
    const double* col = a.d + src * N * N + (size_t)act[row];
    a.r[src * N + (size_t)row] = pairwise_sum([&](int b) { return col[(size_t)act[b] * N]; }, m);
}

// Thread `tid` of workgroup `wg` of `G` on Q of join t: rows wg, wg + G, ..., columns tid, tid + threads, ...
// q = ((m - 2) d_ab - r[a]) - r[b]: two roundings, no FMA
PF_TAXA_HD inline Key qmin_thread(const Args& a, int m, int t, size_t src, int wg, int G, int tid, int threads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    Key best = key_none();
    if (a.flag[src]) return best;
    const size_t N = (size_t)a.N;
    const int32_t* act = active_of(a, src, t);
    const double* d = a.d + src * N * N;
    const double* r = a.r + src * N;
    const double mm2 = (double)(m - 2);
    for (int ra = wg; ra < m; ra += G) {
        const double* row = d + (size_t)act[ra] * N;
        const double rsum = r[ra];
        for (int cb = tid; cb < m; cb += threads) {
            if (cb == ra) continue;
            const double prod = mm2 * row[act[cb]];
            const Key k{(prod - rsum) - r[cb], ra, cb};
            if (key_less(k, best)) best = k;
        }
    }
    return best;
}

// One step of the minimum of keys[0 .. threads) in a workgroup (a barrier stands between two steps): s = the power of
// two >= threads / 2, then s / 2, ..., 1; the result is keys[0].
PF_TAXA_HD inline void reduce_step(Key* keys, int tid, int s, int threads) {
    if (tid < s && tid + s < threads && key_less(keys[tid + s], keys[tid])) keys[tid] = keys[tid + s];
}
PF_TAXA_HD inline int reduce_first_step(int threads) {
    int s = 1;
    while (2 * s < threads) s *= 2;
    return s;
}
// the serial drivers' workgroup minimum: the same steps, thread by thread
inline void reduce_keys_serial(Key* keys, int threads) {
    for (int s = reduce_first_step(threads); s > 0; s >>= 1)
        for (int tid = 0; tid < threads; ++tid) reduce_step(keys, tid, s, threads);
}

// thread `tid` of the join's one workgroup: the minimum of the partial minima tid, tid + threads, ... of G
PF_TAXA_HD inline Key join_thread_key(const Args& a, size_t src, int G, int tid, int threads) {
    Key best = key_none();
    if (a.flag[src]) return best;
    const Key* part = a.part + src * (size_t)a.part_cap;
    for (int g = tid; g < G; g += threads)
        if (key_less(part[g], best)) best = part[g];
    return best;
}

// what one thread works out of the minimum and all threads of the join read (through LDS on the device)
struct Join { int32_t ia, ib, pos_b, ok; double dab; };

// Join t from the minimum of Q: a < b, their slots, dab, the branch lengths; writes the table.  ok = 0: a flagged
// source, or - never with finite input - a minimum outside the matrix (the source is flagged then).
PF_TAXA_HD inline Join join_record(const Args& a, int m, int t, size_t src, Key best) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    Join j{0, 0, 0, 0, 0.0};
    if (a.flag[src]) return j;
    if (best.a < 0 || best.a >= m || best.b < 0 || best.b >= m || best.a == best.b) { a.flag[src] = 1; return j; }
    const size_t N = (size_t)a.N;
    const int32_t* act = active_of(a, src, t);
    const double* r = a.r + src * N;
    const int pa = best.a < best.b ? best.a : best.b, pb = best.a < best.b ? best.b : best.a;
    j.ia = act[pa]; j.ib = act[pb]; j.pos_b = pb; j.ok = 1;
    j.dab = a.d[src * N * N + (size_t)j.ia * N + (size_t)j.ib];
    const double la = 0.5 * j.dab + (r[pa] - r[pb]) / (double)(2 * ((int64_t)m - 2));
    const double lb = j.dab - la;
    const size_t at = src * (size_t)table_len(a.N) + 2 * (size_t)t;
    a.slots[at] = j.ia; a.slots[at + 1] = j.ib;
    a.lengths[at] = la; a.lengths[at + 1] = lb;
    return j;
}

// Thread `tid` of the join's workgroup after join_record (dab comes from `j`: d[ia][ib] is overwritten here): row and
// column ia become the new node's distances dn[k] = 0.5 ((d[ia][k] + d[ib][k]) - dab) for all k < N, d[ia][ia] = 0, and
// position pos_b leaves the list of active slots.  Thread k reads d[ia][k] and d[ib][k] and writes d[ia][k] and
// d[k][ia]; k = ia only writes the zero (it would read d[ib][ia], which thread ib writes).
PF_TAXA_HD inline void join_update(const Args& a, int m, int t, size_t src, const Join& j, int tid, int threads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!j.ok) return;
    const size_t N = (size_t)a.N, ia = (size_t)j.ia, ib = (size_t)j.ib;
    double* d = a.d + src * N * N;
    for (size_t k = (size_t)tid; k < N; k += (size_t)threads) {
        if (k == ia) { d[ia * N + ia] = 0.0; continue; }
        const double dn = 0.5 * ((d[ia * N + k] + d[ib * N + k]) - j.dab);
        d[ia * N + k] = dn;
        d[k * N + ia] = dn;
    }
    const int32_t* act = active_of(a, src, t);
    int32_t* next = a.active + (src * 2 + (size_t)((t + 1) & 1)) * N;
    for (int p = tid; p < m - 1; p += threads) next[p] = act[p + (p >= j.pos_b ? 1 : 0)];
}

// after the last join: the three remaining slots and their branch lengths, as nj_core forms them
PF_TAXA_HD inline void final_record(const Args& a, size_t src) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (a.flag[src]) return;
    const size_t N = (size_t)a.N;
    const int32_t* act = active_of(a, src, a.N - 3);
    const double* d = a.d + src * N * N;
    const size_t i = (size_t)act[0], j = (size_t)act[1], k = (size_t)act[2];
    const size_t at = src * (size_t)table_len(a.N) + 2 * (N - 3);
    a.slots[at] = (int32_t)i; a.slots[at + 1] = (int32_t)j; a.slots[at + 2] = (int32_t)k;
    a.lengths[at] = 0.5 * ((d[i * N + j] + d[i * N + k]) - d[j * N + k]);
    a.lengths[at + 1] = 0.5 * ((d[i * N + j] + d[j * N + k]) - d[i * N + k]);
    a.lengths[at + 2] = 0.5 * ((d[i * N + k] + d[j * N + k]) - d[i * N + j]);
}

// ---- the arrays of a state, listed once: state_arrays (pf_spans.h has the visitors); the staging: staging_arrays -------
using pfspan::Measure;
using pfspan::Carve;
using pfspan::Allocate;

// the scalars of `a`; the state besides the caller's arrays (preds, slots, lengths, flag) follows by state_arrays
inline Args args_of(const float* preds, int N, int part_cap, int32_t* slots, double* lengths, uint8_t* flag) {
    Args a{};
    a.preds = preds; a.slots = slots; a.lengths = lengths; a.flag = flag;
    a.N = N; a.part_cap = part_cap; a.PN = (int64_t)N * (N - 1) / 2;
    return a;
}

template <class V>
inline void state_arrays(V& v, Args& a, size_t B) {
    const size_t n = (size_t)a.N;
    v(a.d, B * n * n);
    v(a.r, B * n);
    v(a.part, B * (size_t)a.part_cap);
    v(a.active, B * 2 * n);
}

// bytes of one source's state on the device
inline size_t state_bytes(int N) {
    Args a = args_of(nullptr, N, Q_GROUPS, nullptr, nullptr, nullptr);
    return pfspan::measure([&](auto& v) { state_arrays(v, a, 1); });
}

// the state of B sources carved from `ws` (8-byte aligned, B * state_bytes(N) bytes)
inline Args carve(char* ws, const float* preds, int B, int N, int32_t* slots, double* lengths, uint8_t* flag) {
    Args a = args_of(preds, N, Q_GROUPS, slots, lengths, flag);
    pfspan::carve(ws, [&](auto& v) { state_arrays(v, a, (size_t)B); });
    return a;
}

// The arrays of a call (pf_nj_joins, pf_bionj_joins) as the caller or the staging of a chunk holds them, and the caller's
// from source b0 on.
struct Tables { const float* preds; int32_t* slots; double* lengths; uint8_t* flag; };
inline Tables chunk_of(const Tables& u, size_t b0, int N) {
    const size_t T = (size_t)table_len(N), PN = (size_t)N * ((size_t)N - 1) / 2;
    return {u.preds + b0 * PN, u.slots + b0 * T, u.lengths + b0 * T, u.flag + b0};
}
// The staging `s` of one chunk of a host call with the caller's arrays `u`: what goes up and what comes down.
template <class V>
inline void staging_arrays(V& v, Tables& s, const Tables& u, size_t chunk, int N) {
    const size_t T = (size_t)table_len(N), PN = (size_t)N * ((size_t)N - 1) / 2;
    v.out(s.lengths, u.lengths, chunk * T);
    v.in(s.preds, u.preds, chunk * PN);
    v.out(s.slots, u.slots, chunk * T);
    v.out(s.flag, u.flag, chunk);
}
// the layout alone, for a visitor with operator() only
using Staging = Tables;
template <class V>
inline void staging_arrays(V& v, Staging& s, size_t chunk, int N) {
    pfspan::StagingOnly<V> only{v};
    staging_arrays(only, s, Tables{}, chunk, N);
}

}  // namespace pfnj
