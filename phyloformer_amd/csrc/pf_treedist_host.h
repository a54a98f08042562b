// Distances between the join tables of one source (pf_join_distances, pf_join_distances_device, pf_join_distances_host;
// DESIGN.md section 35): shared splits (Robinson-Foulds), the Kuhner-Felsenstein branch score and weighted RF of every
// pair of K trees.  The bodies of the kernels of pf_treedist.hip.h as functions of (source, entry or pair, lane).  Plain
// C++, no HIP: pf_hostio.cpp runs them serially as the CPU twin; pf_treedist.hip.h compiles them for the device too
// (PF_TAXA_HD).  phyloformer_amd/treedist.py::join_distances_py is the statement.
//
// The first half IS pfcon's (pf_consensus_host.h), called through a pfcon::Args whose replicates are the K trees: the
// bitset tables with `above` and `leaf_pos` (pfsup's join_ok, join_words, normalise, final_ok; pfcon's branch_at), the
// keys (key_of) and the exact hash table (count_entry: claim, compare by hash and then by all W words, a probe bound).
// Equal splits settle in one slot, so two splits are equal iff their slots are: a slot id depends on who claimed first,
// what is computed from the ids - equal or not - does not.  Per source, with S = N - 3, E = K S, C slots:
//   pfcon's   bits [K][W][S], row [K][N], sizes [K][S], above [K][S], leaf_pos [K][N], hash [E], low [E], slot_of [E],
//             owner [C], tally [C], err
//   idx_slot  int32 [K][S]   a tree's slots in ascending order (distinct within a tree: its splits are)
//   idx_entry int32 [K][S]   ... and the split t of the tree that sits there
// A pair looks split t of tree i up in tree j's index by binary search.  The sums are section 32's: 64 accumulators over
// u = lane, lane + 64, ..., then lane l takes lane l + s for s = 32 .. 1; every product and sum is rounded where written
// (the bodies switch contraction off; a g++ build passes -ffp-contract=off).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pf_consensus_host.h"
#include "pf_spans.h"

namespace pftd {

using pfcon::ERR_FULL;
using pfcon::ERR_TABLE;
using pfcon::NONE;
using pfsup::table_len;
using pfsup::words_of;

constexpr int LANES = 64;
constexpr int MIN_N = 4, MAX_N = 16384, MAX_K = 4096;
// K (N - 3) of one source: entries and slots are int32, as pfcon's; the two caps keep it there, so no call is refused for it
static_assert((int64_t)MAX_K * (MAX_N - 3) <= pfcon::MAX_ENTRIES, "K (N - 3) <= 2^29 follows from MAX_K and MAX_N");

struct Args {
    pfcon::Args c;                  // what pfcon's bodies see: rep_* = the call's tables, R = K; no selection, no results but status
    int32_t *idx_slot, *idx_entry;  // [nb][K][S]
    int32_t* shared;                // [B][K][K]
    double *kf, *wrf;               // [B][K][K] or null (no lengths)
};

// The arrays of a chunk of nb sources; [first_ones, zeros) is filled with 0xff bytes (NONE), [zeros, end) with zeros
// before the chunk runs, what lies before needs no start value.
template <class V>
inline void state_arrays(V& v, Args& a, size_t nb, size_t K, int N, size_t cap) {
    const size_t S = (size_t)N - 3, W = (size_t)words_of(N), E = K * S;
    v(a.c.bits, nb * E * W);
    v(a.c.hash, nb * E);
    v(a.c.row, nb * K * (size_t)N);
    v(a.c.sizes, nb * E);
    v(a.c.above, nb * E);
    v(a.c.leaf_pos, nb * K * (size_t)N);
    v(a.c.low, nb * E);
    v(a.idx_slot, nb * E);
    v(a.idx_entry, nb * E);
    v(a.c.slot_of, nb * E);        // NONE from here
    v(a.c.owner, nb * cap);
    v(a.c.tally, nb * cap);        // zeros from here
    v(a.c.err, nb);
}
inline size_t state_bytes(int N, int64_t K) {
    Args a{};
    pfspan::Measure m;
    state_arrays(m, a, 1, (size_t)K, N, (size_t)pfcon::capacity_of(K * ((int64_t)N - 3)));
    return m.bytes;
}
inline size_t min_state_bytes(int N) { return state_bytes(N, 1); }

// The arrays of a call (pf_join_distances) as the caller or the staging holds them.
struct Tables {
    const int32_t* slots; const double* lengths; const uint8_t* flag;
    int32_t* shared; double *kf, *wrf; uint8_t* status;
};
// The staging `s` of a whole host call with the caller's arrays `u`.  Without the caller's lengths there are none and no
// kf / wrf, with them both are required; a null flag keeps its span.
template <class V>
inline void staging_arrays(V& v, Tables& s, const Tables& u, size_t B, size_t K, int N) {
    const size_t T = (size_t)table_len(N);
    const pfspan::Need lengths = u.lengths ? pfspan::REQUIRED : pfspan::ABSENT;
    v.in(s.lengths, u.lengths, B * K * T, lengths);
    v.out(s.kf, u.kf, B * K * K, lengths);
    v.out(s.wrf, u.wrf, B * K * K, lengths);
    v.in(s.slots, u.slots, B * K * T);
    v.out(s.shared, u.shared, B * K * K);
    v.in(s.flag, u.flag, B * K, pfspan::OPTIONAL);
    v.out(s.status, u.status, B);
}

PF_TAXA_HD inline int trees_of(const Args& a) { return a.c.R; }
PF_TAXA_HD inline int64_t pairs_of(int K) { return (int64_t)K * (K - 1) / 2; }

// ---- k_td_index: one thread per entry ------------------------------------------------------------------------------------

// Entry e = (tree r, split t): its slot's rank among the tree's S slots, by counting; the slot and t go there.
PF_TAXA_HD inline void index_entry(const Args& a, int src, int64_t e) {
    const int S = a.c.N - 3, r = (int)(e / S), t = (int)(e % S);
    if (a.c.err[src]) return;
    if (pfcon::flagged(a.c, src, r)) return;
    const size_t tree = (size_t)src * pfcon::entries_of(a.c) + (size_t)r * (size_t)S;
    const int32_t* slot_of = a.c.slot_of + tree;
    const int32_t mine = slot_of[t];
    int rank = 0;
    for (int k = 0; k < S; ++k) rank += slot_of[k] < mine;
    a.idx_slot[tree + (size_t)rank] = mine;
    a.idx_entry[tree + (size_t)rank] = t;
}

// ---- k_td_pairs: one wave per pair ---------------------------------------------------------------------------------------

// pair p = 0 .. K (K - 1) / 2 - 1 in the order (0, 1), (0, 2), ..., (1, 2), ...
PF_TAXA_HD inline int64_t pair_start(int64_t i, int K) { return i * (2 * (int64_t)K - i - 1) / 2; }
PF_TAXA_HD inline void pair_of(int64_t p, int K, int* i, int* j) {
    const double k2 = 2.0 * (double)K - 1.0;
    int64_t r = (int64_t)((k2 - sqrt(k2 * k2 - 8.0 * (double)p)) / 2.0);
    if (r < 0) r = 0;
    if (r > K - 2) r = K - 2;
    while (r > 0 && pair_start(r, K) > p) --r;
    while (r < K - 2 && pair_start(r + 1, K) <= p) ++r;
    *i = (int)r;
    *j = (int)(p - pair_start(r, K) + r + 1);
}

// the split of tree r that sits in `slot`, or NONE
PF_TAXA_HD inline int32_t find(const Args& a, int src, int r, int32_t slot) {
    const int S = a.c.N - 3;
    const size_t tree = (size_t)src * pfcon::entries_of(a.c) + (size_t)r * (size_t)S;
    const int32_t* s = a.idx_slot + tree;
    int lo = 0, hi = S;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (s[mid] < slot) lo = mid + 1;
        else hi = mid;
    }
    return lo < S && s[lo] == slot ? a.idx_entry[tree + (size_t)lo] : NONE;
}

struct Acc { double sq, ab; int32_t hits; };

PF_TAXA_HD inline void acc_take(Acc& a, double d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double q = d * d;
    a.sq = a.sq + q;
    a.ab = a.ab + fabs(d);
}

// lane l takes lane l + s
PF_TAXA_HD inline void acc_merge(Acc& a, const Acc& o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    a.sq = a.sq + o.sq;
    a.ab = a.ab + o.ab;
    a.hits += o.hits;
}

// lane `lane` of pair i < j of chunk source src: the terms u = lane, lane + 64, ... of the statement's list (without
// lengths: phase A's hits alone)
PF_TAXA_HD inline Acc pair_lane(const Args& a, int src, int i, int j, int lane) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int N = a.c.N, S = N - 3;
    const bool lengths = a.c.rep_lengths != nullptr;
    const size_t base = (size_t)src * pfcon::entries_of(a.c);
    const size_t ti = pfcon::tree_index(a.c, src, i), tj = pfcon::tree_index(a.c, src, j);
    const int32_t *slot_i = a.c.slot_of + base + (size_t)i * (size_t)S, *slot_j = a.c.slot_of + base + (size_t)j * (size_t)S;
    const int32_t *above_i = a.c.above + ti * (size_t)S, *above_j = a.c.above + tj * (size_t)S;
    const int32_t *leaf_i = a.c.leaf_pos + ti * (size_t)N, *leaf_j = a.c.leaf_pos + tj * (size_t)N;
    const double* li = lengths ? pfcon::lengths_of(a.c, src, i) : nullptr;
    const double* lj = lengths ? pfcon::lengths_of(a.c, src, j) : nullptr;
    const int U = lengths ? 2 * S + N : S;
    Acc acc{0.0, 0.0, 0};
    for (int u = lane; u < U; u += LANES) {
        double d;
        if (u < S) {
            const int32_t f = find(a, src, j, slot_i[u]);
            acc.hits += f != NONE;
            if (!lengths) continue;
            const double b = f != NONE ? lj[above_j[f]] : 0.0;
            d = li[above_i[u]] - b;
        } else if (u < 2 * S) {
            const int t = u - S;
            d = find(a, src, i, slot_j[t]) != NONE ? 0.0 : 0.0 - lj[above_j[t]];
        } else {
            const int x = u - 2 * S;
            d = li[leaf_i[x]] - lj[leaf_j[x]];
        }
        acc_take(acc, d);
    }
    return acc;
}

// lane 0's sums of pair i < j into (i, j) and (j, i)
PF_TAXA_HD inline void pair_store(const Args& a, int src, int i, int j, const Acc& acc) {
    const size_t K = (size_t)trees_of(a), o = (size_t)(a.c.b0 + src) * K * K;
    const size_t ij = o + (size_t)i * K + (size_t)j, ji = o + (size_t)j * K + (size_t)i;
    a.shared[ij] = a.shared[ji] = acc.hits;
    if (!a.c.rep_lengths) return;
    a.kf[ij] = a.kf[ji] = sqrt(acc.sq);
    a.wrf[ij] = a.wrf[ji] = acc.ab;
}

// does pair (i, j) of chunk source src have a value?
PF_TAXA_HD inline bool pair_runs(const Args& a, int src, int i, int j) {
    return !a.c.err[src] && !pfcon::flagged(a.c, src, i) && !pfcon::flagged(a.c, src, j);
}

// ---- k_td_finish: one thread per cell ------------------------------------------------------------------------------------

// Cell u = i K + j: the diagonal and the cells of a flagged tree; u = 0 the source's status besides.  A source with an
// error keeps the zeros its results were filled with.
PF_TAXA_HD inline void finish_cell(const Args& a, int src, int64_t u) {
    const int K = trees_of(a), err = a.c.err[src];
    if (u == 0) a.c.status[a.c.b0 + src] = (uint8_t)(err & ERR_TABLE ? 1 : err ? 2 : 0);
    if (err) return;
    const int i = (int)(u / K), j = (int)(u % K);
    const bool none = pfcon::flagged(a.c, src, i) || pfcon::flagged(a.c, src, j);
    if (!none && i != j) return;
    const size_t o = (size_t)(a.c.b0 + src) * (size_t)K * (size_t)K + (size_t)u;
    a.shared[o] = none ? -1 : a.c.N - 3;
    if (!a.c.rep_lengths) return;
    a.kf[o] = a.wrf[o] = none ? __builtin_nan("") : 0.0;
}

// ---- the serial run of the bodies (the CPU twin) -------------------------------------------------------------------------

// the wave of pair (i, j): 64 lanes one after the other, then the merges in the shuffles' order
inline void serial_pair(const Args& a, int src, int i, int j) {
    if (!pair_runs(a, src, i, j)) return;
    Acc acc[LANES];
    for (int lane = 0; lane < LANES; ++lane) acc[lane] = pair_lane(a, src, i, j, lane);
    for (int s = LANES / 2; s > 0; s >>= 1)
        for (int lane = 0; lane < s; ++lane) acc_merge(acc[lane], acc[lane + s]);
    pair_store(a, src, i, j, acc[0]);
}

// One chunk source, start to finish; its state holds the start values (state_arrays), its results zeros.
inline void serial_source(const Args& a, int src) {
    const int K = trees_of(a);
    const int64_t E = (int64_t)pfcon::entries_of(a.c);
    for (int r = 0; r < K; ++r)
        if (!pfcon::flagged(a.c, src, r) && !pfcon::serial_tree(a.c, src, r)) a.c.err[src] |= ERR_TABLE;
    for (int64_t e = 0; e < E; ++e) pfcon::keys_entry(a.c, src, e);
    for (int64_t e = 0; e < E; ++e) pfcon::count_entry(a.c, pfcon::PlainTable{}, src, e);
    for (int64_t e = 0; e < E; ++e) index_entry(a, src, e);
    for (int64_t p = 0; p < pairs_of(K); ++p) {
        int i = 0, j = 0;
        pair_of(p, K, &i, &j);
        serial_pair(a, src, i, j);
    }
    for (int64_t u = 0; u < (int64_t)K * K; ++u) finish_cell(a, src, u);
}

}  // namespace pftd
