// Majority-rule consensus of replicate join tables (pf_join_consensus, pf_join_consensus_device, pf_join_consensus_host;
// DESIGN.md section 25): the bodies of the kernels of pf_consensus.hip.h as functions of (tree or source, thread,
// threads).  Plain C++, no HIP: pf_hostio.cpp runs them serially (one thread) as the CPU twin; pf_consensus.hip.h
// compiles them for the device too (PF_TAXA_HD).  phyloformer_amd/consensus.py::join_consensus is the statement.
//
// The split builder is pfsup's (join_ok, join_words, normalise; word-major bits[w * S + t]).  Per source, with S = N - 3
// splits per tree, W = ceil(N / 64) words per split, R replicates, E = R S split entries (entry e = r S + t) and a hash
// table of C slots (a power of two >= 2 E):
//   bits      uint64 [R][W][S]   the bitset tables of the replicates (a flagged replicate's is never written or read)
//   row       int32  [R][N]      pfsup's row bookkeeping
//   sizes     int32  [R][S]      sequences of every split
//   above     int32  [R][S]      position in the table's lengths of the branch above join t's cluster
//   leaf_pos  int32  [R][N]      ... and above leaf x
//   hash      uint64 [E]         64-bit mix of the split's words
//   low       int32  [E]         its lowest member
//   slot_of   int32  [E]         the slot the entry settled in (NONE: a flagged replicate's, or none found)
//   owner     int32  [C]         the entry that claimed the slot, NONE = empty; slots are never emptied, so two equal
//                                splits always settle in one slot: the counts do not depend on the scheduling
//   tally     int32  [C]         entries settled in the slot: c(s)
//   rank_of   int32  [C]         the canonical rank of a selected slot's split, NONE otherwise
//   sel       int32  [S]         the selected slots, in any order; order [S]: the slot of every rank
//   cbits     uint64 [W][S]      the selected splits in rank order, word-major like a tree's table
//   lens      double [S][R]      branch length of split `rank` in replicate r; present uint8 [S][R] marks the entries
//   nsel      int32              selected slots;  err int32: ERR_* bits
// Everything but the sums is an integer; the sums run in ascending replicate order and hold no product.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pf_spans.h"
#include "pf_support_host.h"

namespace pfcon {

using pfsup::popc;
using pfsup::table_len;
using pfsup::words_of;

constexpr int TILE = 16;                // selected splits of one workgroup of the nesting kernel
constexpr int32_t NONE = -1;
constexpr int ERR_TABLE = 1;            // an unflagged table is no join table (status 1)
constexpr int ERR_FULL = 2;             // a split found no slot in the hash table (status 2; not at the library's capacity)
constexpr int ERR_SELECT = 4;           // more than N - 3 selected splits, or two with one (size, lowest member) (status 2)
constexpr int64_t MAX_ENTRIES = (int64_t)1 << 29;   // R (N - 3) of one source: entries and slots are int32

// The library's capacity: the least power of two >= 2 E.
inline int64_t capacity_of(int64_t entries) {
    int64_t c = 2;
    while (c < 2 * entries) c *= 2;
    return c;
}

struct Args {
    const int32_t* rep_slots;    // [B][R][T]
    const double* rep_lengths;   // [B][R][T] or null
    const uint8_t* rep_flag;     // [B][R] or null
    // the chunk's state, source after source (list `state_arrays`)
    uint64_t *bits, *hash, *cbits;
    double* lens;
    int32_t *row, *sizes, *above, *leaf_pos, *low, *slot_of, *owner, *rank_of, *tally, *sel, *order, *nsel, *err;
    uint8_t* present;
    // the results, [B] in front
    int32_t *n_splits, *count, *size, *parent, *leaf_parent;   // [1], [S], [S], [S], [N]
    double *split_length, *leaf_length;                        // [S], [N] or null
    uint8_t* status;
    int N, R, percent;
    int b0, nb;                  // the chunk's sources b0 .. b0 + nb - 1
    int64_t cap;                 // slots of a source's hash table (a power of two)
};

// The arrays of a chunk of nb sources; [first_ones, zeros) is filled with 0xff bytes (NONE), [zeros, end) with zeros
// before the chunk runs, what lies before needs no start value.
template <class V>
inline void state_arrays(V& v, Args& a, size_t nb, size_t R, int N, size_t cap, bool lengths) {
    const size_t S = (size_t)N - 3, W = (size_t)words_of(N), E = R * S;
    v(a.bits, nb * E * W);
    v(a.hash, nb * E);
    v(a.cbits, nb * S * W);
    v(a.lens, lengths ? nb * S * R : 0);
    v(a.row, nb * R * (size_t)N);
    v(a.sizes, nb * E);
    v(a.above, nb * E);
    v(a.leaf_pos, nb * R * (size_t)N);
    v(a.low, nb * E);
    v(a.sel, nb * S);
    v(a.order, nb * S);
    v(a.slot_of, nb * E);          // NONE from here
    v(a.owner, nb * cap);
    v(a.rank_of, nb * cap);
    v(a.tally, nb * cap);          // zeros from here
    v(a.nsel, nb);
    v(a.err, nb);
    v(a.present, lengths ? nb * S * R : 0);
}
inline size_t state_bytes(int N, int64_t R, bool lengths = true) {
    Args a{};
    pfspan::Measure m;
    state_arrays(m, a, 1, (size_t)R, N, (size_t)capacity_of(R * ((int64_t)N - 3)), lengths);
    return m.bytes;
}
inline size_t min_state_bytes(int N) { return state_bytes(N, 1); }

// The arrays of a call (pf_join_consensus) as the caller or the staging holds them.
struct Tables {
    const int32_t* rep; const double* lengths; const uint8_t* flag;
    int32_t *n_splits, *count, *size, *parent; double* split_length; int32_t* leaf_parent; double* leaf_length; uint8_t* status;
};
// The staging `s` of a whole host call with the caller's arrays `u`: what goes up and what comes down.  Without the
// caller's rep_lengths there are no lengths, with them both length results are required; a null rep_flag keeps its span.
template <class V>
inline void staging_arrays(V& v, Tables& s, const Tables& u, size_t B, size_t R, int N) {
    const size_t T = (size_t)table_len(N), S = (size_t)N - 3;
    const pfspan::Need lengths = u.lengths ? pfspan::REQUIRED : pfspan::ABSENT;
    v.in(s.lengths, u.lengths, B * R * T, lengths);
    v.out(s.split_length, u.split_length, B * S, lengths);
    v.out(s.leaf_length, u.leaf_length, B * (size_t)N, lengths);
    v.in(s.rep, u.rep, B * R * T);
    v.out(s.n_splits, u.n_splits, B);
    v.out(s.count, u.count, B * S);
    v.out(s.size, u.size, B * S);
    v.out(s.parent, u.parent, B * S);
    v.out(s.leaf_parent, u.leaf_parent, B * (size_t)N);
    v.in(s.flag, u.flag, B * R, pfspan::OPTIONAL);
    v.out(s.status, u.status, B);
}

// ---- where the arrays of chunk source src, replicate r are ------------------------------------------------------------

PF_TAXA_HD inline size_t entries_of(const Args& a) { return (size_t)a.R * (size_t)(a.N - 3); }
PF_TAXA_HD inline size_t tree_index(const Args& a, int src, int r) { return (size_t)src * (size_t)a.R + (size_t)r; }
PF_TAXA_HD inline uint64_t* bits_of(const Args& a, int src, int r) {
    return a.bits + tree_index(a, src, r) * (size_t)(a.N - 3) * (size_t)words_of(a.N);
}
PF_TAXA_HD inline uint64_t* cbits_of(const Args& a, int src) { return a.cbits + (size_t)src * (size_t)(a.N - 3) * (size_t)words_of(a.N); }
PF_TAXA_HD inline size_t global_tree(const Args& a, int src, int r) { return (size_t)(a.b0 + src) * (size_t)a.R + (size_t)r; }
PF_TAXA_HD inline const int32_t* slots_of(const Args& a, int src, int r) { return a.rep_slots + global_tree(a, src, r) * (size_t)table_len(a.N); }
PF_TAXA_HD inline const double* lengths_of(const Args& a, int src, int r) { return a.rep_lengths + global_tree(a, src, r) * (size_t)table_len(a.N); }
PF_TAXA_HD inline bool flagged(const Args& a, int src, int r) { return a.rep_flag && a.rep_flag[global_tree(a, src, r)]; }

// ---- k_con_splits: one workgroup per tree ------------------------------------------------------------------------------

// What join t (or, t = S, the trifurcation) consumes: the cluster in `slot`, whose row is r, has its branch at position p.
PF_TAXA_HD inline void branch_at(int32_t* above, int32_t* leaf_pos, int32_t slot, int32_t r, int p) {
    if (r >= 0) above[r] = p;
    else leaf_pos[slot] = p;
}

// ---- k_con_keys: one thread per entry ----------------------------------------------------------------------------------

PF_TAXA_HD inline uint64_t mix(uint64_t h, uint64_t x) {
    h = (h ^ x) * 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 29);
}

// hash and lowest member of split t of a tree (its size is normalise's)
PF_TAXA_HD inline void key_of(const uint64_t* bits, int S, int W, int t, uint64_t* hash, int32_t* low) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    int32_t first = -1;
    for (int w = 0; w < W; ++w) {
        const uint64_t x = bits[(size_t)w * (size_t)S + (size_t)t];
        h = mix(h, x);
        if (first < 0 && x) first = w * 64 + __builtin_ctzll(x);
    }
    *hash = h;
    *low = first;
}

PF_TAXA_HD inline void keys_entry(const Args& a, int src, int64_t e) {
    const int S = a.N - 3, W = words_of(a.N), r = (int)(e / S), t = (int)(e % S);
    if (a.err[src] & ERR_TABLE) return;
    if (flagged(a, src, r)) return;
    const size_t o = (size_t)src * entries_of(a) + (size_t)e;
    key_of(bits_of(a, src, r), S, W, t, a.hash + o, a.low + o);
}

// ---- k_con_count: one thread per entry ---------------------------------------------------------------------------------

// How the table is claimed and counted and how bits of a source's error word are set - several threads may do either -:
// plainly on the CPU, with vector atomics on the device (pf_consensus.hip.h).
struct PlainTable {
    PF_TAXA_HD void raise(int32_t* err, int bits) const { *err |= bits; }
    PF_TAXA_HD int32_t claim(int32_t* owner, int32_t e) const {
        const int32_t old = *owner;
        if (old == NONE) *owner = e;
        return old;
    }
    PF_TAXA_HD void add(int32_t* tally) const { ++*tally; }
};

PF_TAXA_HD inline bool same_split(const Args& a, int src, int64_t e, int64_t o) {
    const int S = a.N - 3, W = words_of(a.N);
    const uint64_t* x = bits_of(a, src, (int)(e / S)) + e % S;
    const uint64_t* y = bits_of(a, src, (int)(o / S)) + o % S;
    for (int w = 0; w < W; ++w)
        if (x[(size_t)w * (size_t)S] != y[(size_t)w * (size_t)S]) return false;
    return true;
}

// Entry e probes from its hash: an empty slot is claimed, an occupied one is compared by hash and then by all W words.
// At most `cap` probes: an entry that finds no slot raises ERR_FULL and the loop ends.
template <class Table>
PF_TAXA_HD inline void count_entry(const Args& a, const Table& table, int src, int64_t e) {
    const int S = a.N - 3, r = (int)(e / S);
    if (a.err[src] & ERR_TABLE) return;
    if (flagged(a, src, r)) return;
    const size_t base = (size_t)src * entries_of(a);
    int32_t* owner = a.owner + (size_t)src * (size_t)a.cap;
    int32_t* tally = a.tally + (size_t)src * (size_t)a.cap;
    const uint64_t h = a.hash[base + (size_t)e];
    for (int64_t probe = 0; probe < a.cap; ++probe) {
        const int64_t slot = (int64_t)((h + (uint64_t)probe) & (uint64_t)(a.cap - 1));
        int32_t o = owner[slot];
        if (o == NONE) {
            o = table.claim(owner + slot, (int32_t)e);
            if (o == NONE) o = (int32_t)e;                        // (claimed)
        }
        if (o == (int32_t)e || (a.hash[base + (size_t)o] == h && same_split(a, src, e, o))) {
            table.add(tally + slot);
            a.slot_of[base + (size_t)e] = (int32_t)slot;
            return;
        }
    }
    table.raise(a.err + src, ERR_FULL);
}

// ---- k_con_select: one thread per slot;  k_con_rank: one thread per selected slot --------------------------------------

// is a split in c of R replicates selected at `percent`?  (strictly: exactly half at 50 is not)
PF_TAXA_HD inline bool selected(int32_t c, int R, int percent) { return 100 * (int64_t)c > (int64_t)percent * (int64_t)R; }

// `at`: the position the slot takes in sel (the device: an atomic counter's old value)
template <class Table>
PF_TAXA_HD inline void select_put(const Args& a, const Table& table, int src, int64_t slot, int32_t at) {
    const int S = a.N - 3;
    if (at < S) a.sel[(size_t)src * (size_t)S + (size_t)at] = (int32_t)slot;
    else table.raise(a.err + src, ERR_SELECT);
}

PF_TAXA_HD inline bool select_slot(const Args& a, int src, int64_t slot) {
    if (a.err[src]) return false;
    const size_t o = (size_t)src * (size_t)a.cap + (size_t)slot;
    return a.owner[o] != NONE && selected(a.tally[o], a.R, a.percent);
}

PF_TAXA_HD inline int selected_count(const Args& a, int src) {
    const int m = a.nsel[src], S = a.N - 3;
    return m < S ? m : S;
}

// Selected slot i of sel: its rank = the selected splits with a smaller (size, lowest member); the slot's rank, the
// rank's slot and the split's words in rank order.  Two equal keys: ERR_SELECT.
template <class Table>
PF_TAXA_HD inline void rank_selected(const Args& a, const Table& table, int src, int i) {
    const int S = a.N - 3, W = words_of(a.N), M = selected_count(a, src);
    if (a.err[src] & (ERR_TABLE | ERR_FULL)) return;
    const size_t base = (size_t)src * entries_of(a);
    const int32_t* sel = a.sel + (size_t)src * (size_t)S;
    const int32_t* owner = a.owner + (size_t)src * (size_t)a.cap;
    const int32_t e = owner[sel[i]];
    const int32_t size = a.sizes[base + (size_t)e], low = a.low[base + (size_t)e];
    int rank = 0;
    bool twice = false;
    for (int j = 0; j < M; ++j) {
        const int32_t f = owner[sel[j]];
        const int32_t fs = a.sizes[base + (size_t)f], fl = a.low[base + (size_t)f];
        rank += fs < size || (fs == size && fl < low);
        twice |= j != i && fs == size && fl == low;
    }
    if (twice) { table.raise(a.err + src, ERR_SELECT); return; }
    a.rank_of[(size_t)src * (size_t)a.cap + (size_t)sel[i]] = rank;
    a.order[(size_t)src * (size_t)S + (size_t)rank] = sel[i];
    const uint64_t* x = bits_of(a, src, e / S) + e % S;
    uint64_t* c = cbits_of(a, src) + rank;
    for (int w = 0; w < W; ++w) c[(size_t)w * (size_t)S] = x[(size_t)w * (size_t)S];
}

// ---- k_con_nest: a tile of selected splits against the candidates of larger rank ---------------------------------------

// The tile's words into tile[TILE][W] (zeros beyond the last selected split), thread by thread
PF_TAXA_HD inline void tile_load(uint64_t* tile, const uint64_t* cbits, int S, int W, int M, int t0, int tid, int threads) {
    for (int e = tid; e < TILE * W; e += threads) {
        const int k = e / W, w = e % W;
        tile[e] = t0 + k < M ? cbits[(size_t)w * (size_t)S + (size_t)(t0 + k)] : 0;
    }
}

// best[k] = the least candidate j = t0 + 1 + tid, + threads, ... with j > t0 + k and split_j >= tile split k; M: none.
// Every candidate word is loaded once and meets the whole tile.
PF_TAXA_HD inline void nest_thread(const uint64_t* tile, const uint64_t* cbits, int S, int W, int M, int t0, int tid, int threads, int* best) {
    for (int k = 0; k < TILE; ++k) best[k] = M;
    for (int j = t0 + 1 + tid; j < M; j += threads) {
        uint64_t out[TILE];
        for (int k = 0; k < TILE; ++k) out[k] = 0;
        for (int w = 0; w < W; ++w) {
            const uint64_t x = ~cbits[(size_t)w * (size_t)S + (size_t)j];
            for (int k = 0; k < TILE; ++k) out[k] |= tile[k * W + w] & x;
        }
        for (int k = 0; k < TILE; ++k)
            if (out[k] == 0 && j > t0 + k && j < best[k]) best[k] = j;
    }
}

// the results of rank i whose parent search gave `best`
PF_TAXA_HD inline void nest_put(const Args& a, int src, int i, int best) {
    const int S = a.N - 3, M = selected_count(a, src);
    const size_t o = (size_t)(a.b0 + src) * (size_t)S + (size_t)i;
    const int32_t slot = a.order[(size_t)src * (size_t)S + (size_t)i];
    const size_t at = (size_t)src * (size_t)a.cap + (size_t)slot;
    a.parent[o] = best < M ? best : -1;
    a.count[o] = a.tally[at];
    a.size[o] = a.sizes[(size_t)src * entries_of(a) + (size_t)a.owner[at]];
}

// leaf x: the least rank whose split holds it (ranks ascend by size: the smallest cluster around the leaf)
PF_TAXA_HD inline void nest_leaf(const Args& a, int src, int x) {
    const int S = a.N - 3, M = selected_count(a, src);
    const uint64_t* c = cbits_of(a, src) + (size_t)(x >> 6) * (size_t)S;
    int32_t p = -1;
    for (int j = 0; j < M; ++j)
        if (c[j] >> (x & 63) & 1) { p = j; break; }
    a.leaf_parent[(size_t)(a.b0 + src) * (size_t)a.N + (size_t)x] = p;
}

// ---- k_con_lengths: one thread per entry;  k_con_sums: one thread per selected split and per leaf ----------------------

PF_TAXA_HD inline void length_entry(const Args& a, int src, int64_t e) {
    const int S = a.N - 3, r = (int)(e / S);
    if (a.err[src] || flagged(a, src, r)) return;
    const size_t o = (size_t)src * entries_of(a) + (size_t)e;
    const int32_t slot = a.slot_of[o];
    if (slot == NONE) return;
    const int32_t rank = a.rank_of[(size_t)src * (size_t)a.cap + (size_t)slot];
    if (rank == NONE) return;
    const size_t at = ((size_t)src * (size_t)S + (size_t)rank) * (size_t)a.R + (size_t)r;
    a.lens[at] = lengths_of(a, src, r)[a.above[o]];
    a.present[at] = 1;
}

PF_TAXA_HD inline void sum_split(const Args& a, int src, int i) {
    const int S = a.N - 3;
    const size_t at = ((size_t)src * (size_t)S + (size_t)i) * (size_t)a.R;
    double s = 0.0;
    int c = 0;
    for (int r = 0; r < a.R; ++r)
        if (a.present[at + (size_t)r]) { s += a.lens[at + (size_t)r]; ++c; }
    a.split_length[(size_t)(a.b0 + src) * (size_t)S + (size_t)i] = s / (double)c;
}

PF_TAXA_HD inline void sum_leaf(const Args& a, int src, int x) {
    double s = 0.0;
    int v = 0;
    for (int r = 0; r < a.R; ++r)
        if (!flagged(a, src, r)) { s += lengths_of(a, src, r)[a.leaf_pos[tree_index(a, src, r) * (size_t)a.N + (size_t)x]]; ++v; }
    a.leaf_length[(size_t)(a.b0 + src) * (size_t)a.N + (size_t)x] = v ? s / (double)v : 0.0;
}

// Thread u of a source's last launch: u < S a selected split's mean, S <= u < S + N a leaf's, and u = 0 the source's
// n_splits and status besides.  A source with an error keeps the zeros its results were filled with.
PF_TAXA_HD inline void finish_thread(const Args& a, int src, int u) {
    const int S = a.N - 3, err = a.err[src];
    if (u == 0) {
        a.status[a.b0 + src] = (uint8_t)(err & ERR_TABLE ? 1 : err ? 2 : 0);
        a.n_splits[a.b0 + src] = err ? 0 : selected_count(a, src);
    }
    if (err || !a.rep_lengths) return;
    if (u < S) {
        if (u < selected_count(a, src)) sum_split(a, src, u);
    } else if (u < S + a.N) {
        sum_leaf(a, src, u - S);
    }
}

// ---- the serial run of the bodies (the CPU twin; threads = 1) ----------------------------------------------------------

// replicate r of chunk source src; false: no join table
inline bool serial_tree(const Args& a, int src, int r) {
    const int N = a.N, S = N - 3, W = words_of(N);
    const int32_t* slots = slots_of(a, src, r);
    uint64_t* bits = bits_of(a, src, r);
    const size_t k = tree_index(a, src, r);
    int32_t *row = a.row + k * (size_t)N, *above = a.above + k * (size_t)S, *leaf_pos = a.leaf_pos + k * (size_t)N;
    pfsup::rows_init(row, N, 0, 1);
    for (int t = 0; t < S; ++t) {
        const int32_t sa = slots[2 * t], sb = slots[2 * t + 1];
        int32_t ra = 0, rb = 0;
        if (!pfsup::join_ok(pfsup::PlainRows{row}, N, sa, sb, &ra, &rb)) return false;
        pfsup::join_words(bits, S, W, t, sa, ra, sb, rb, 0, 1);
        branch_at(above, leaf_pos, sa, ra, 2 * t);
        branch_at(above, leaf_pos, sb, rb, 2 * t + 1);
        row[sa] = t;
        row[sb] = pfsup::DEAD;
    }
    if (!pfsup::final_ok(pfsup::PlainRows{row}, N, slots + 2 * (size_t)S)) return false;
    for (int i = 0; i < 3; ++i) branch_at(above, leaf_pos, slots[2 * S + i], row[slots[2 * S + i]], 2 * S + i);
    pfsup::normalise(bits, S, W, N, a.sizes + k * (size_t)S, 0, 1);
    return true;
}

// One chunk source, start to finish; its state holds the start values (state_arrays), its results zeros.
inline void serial_source(const Args& a, int src, uint64_t* tile) {
    const int N = a.N, S = N - 3, W = words_of(N);
    const int64_t E = (int64_t)entries_of(a);
    for (int r = 0; r < a.R; ++r)
        if (!flagged(a, src, r) && !serial_tree(a, src, r)) a.err[src] |= ERR_TABLE;
    for (int64_t e = 0; e < E; ++e) keys_entry(a, src, e);
    for (int64_t e = 0; e < E; ++e) count_entry(a, PlainTable{}, src, e);
    for (int64_t slot = 0; slot < a.cap; ++slot)
        if (select_slot(a, src, slot)) select_put(a, PlainTable{}, src, slot, a.nsel[src]++);
    if (!a.err[src])
        for (int i = 0, M = selected_count(a, src); i < M; ++i) rank_selected(a, PlainTable{}, src, i);
    if (!a.err[src]) {
        const int M = selected_count(a, src);
        for (int t0 = 0; t0 < M; t0 += TILE) {
            int best[TILE];
            tile_load(tile, cbits_of(a, src), S, W, M, t0, 0, 1);
            nest_thread(tile, cbits_of(a, src), S, W, M, t0, 0, 1, best);
            for (int k = 0; k < TILE && t0 + k < M; ++k) nest_put(a, src, t0 + k, best[k]);
        }
        for (int x = 0; x < N; ++x) nest_leaf(a, src, x);
        if (a.rep_lengths)
            for (int64_t e = 0; e < E; ++e) length_entry(a, src, e);
    }
    for (int u = 0; u < S + N; ++u) finish_thread(a, src, u);
}

}  // namespace pfcon
