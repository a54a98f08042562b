// The bodies of the consensus kernels (phyloformer_amd/csrc/pf_consensus_host.h) run on the CPU in the kernels' own
// geometry - workgroups of `threads` threads, one after the other, the entries of the counting kernel in a scrambled
// order - with every array allocated at its exact size, for AddressSanitizer / UBSan (tests/test_consensus_native.py).
// One source:
//   pf_consensus_main N R threads percent cap tables.bin lengths.bin flags.bin out.bin
// tables.bin: int32 [R][2 (N - 3) + 3]; lengths.bin: double [R][2 (N - 3) + 3]; flags.bin: uint8 [R]; cap: slots of the
// hash table, a power of two (0: the library's).
// out.bin: n_splits int32, count / size / parent int32 [N - 3], leaf_parent int32 [N], split_length double [N - 3],
// leaf_length double [N], status uint8.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_consensus_host.h"

using namespace pfcon;

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(T), v.size(), f);
    fclose(f);
    return got == v.size();
}

// k_con_splits' workgroup for replicate r
static void splits_group(const Args& a, int r, int threads) {
    const int N = a.N, S = N - 3, W = words_of(N);
    if (flagged(a, 0, r)) return;
    const int32_t* slots = slots_of(a, 0, r);
    uint64_t* bits = bits_of(a, 0, r);
    const size_t k = tree_index(a, 0, r);
    int32_t *row = a.row + k * (size_t)N, *above = a.above + k * (size_t)S, *leaf_pos = a.leaf_pos + k * (size_t)N;
    for (int tid = 0; tid < threads; ++tid) pfsup::rows_init(row, N, tid, threads);
    for (int t = 0; t < S; ++t) {
        const int32_t sa = slots[2 * t], sb = slots[2 * t + 1];
        int32_t ra = 0, rb = 0;
        if (!pfsup::join_ok(pfsup::PlainRows{row}, N, sa, sb, &ra, &rb)) { a.err[0] |= ERR_TABLE; return; }
        for (int tid = threads - 1; tid >= 0; --tid) pfsup::join_words(bits, S, W, t, sa, ra, sb, rb, tid, threads);
        branch_at(above, leaf_pos, sa, ra, 2 * t);
        branch_at(above, leaf_pos, sb, rb, 2 * t + 1);
        row[sa] = t;
        row[sb] = pfsup::DEAD;
    }
    if (!pfsup::final_ok(pfsup::PlainRows{row}, N, slots + 2 * (size_t)S)) { a.err[0] |= ERR_TABLE; return; }
    for (int tid = 0; tid < 3; ++tid) branch_at(above, leaf_pos, slots[2 * S + tid], row[slots[2 * S + tid]], 2 * S + tid);
    for (int tid = 0; tid < threads; ++tid) pfsup::normalise(bits, S, W, N, a.sizes + k * (size_t)S, tid, threads);
}

// k_con_nest's workgroup for the tile at t0
static void nest_group(const Args& a, int t0, int threads, uint64_t* tile) {
    const int S = a.N - 3, W = words_of(a.N), M = selected_count(a, 0);
    if (a.err[0] || t0 >= M) return;
    for (int tid = 0; tid < threads; ++tid) tile_load(tile, cbits_of(a, 0), S, W, M, t0, tid, threads);
    int all[TILE];
    for (int k = 0; k < TILE; ++k) all[k] = M;
    for (int tid = threads - 1; tid >= 0; --tid) {
        int best[TILE];
        nest_thread(tile, cbits_of(a, 0), S, W, M, t0, tid, threads, best);
        for (int k = 0; k < TILE; ++k) all[k] = std::min(all[k], best[k]);
    }
    for (int tid = 0; tid < TILE && t0 + tid < M; ++tid) nest_put(a, 0, t0 + tid, all[tid]);
}

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int N = atoi(argv[1]), R = atoi(argv[2]), threads = atoi(argv[3]), percent = atoi(argv[4]);
    const long long want_cap = atoll(argv[5]);
    if (N < 4 || R < 1 || threads < 1 || want_cap < 0 || (want_cap & (want_cap - 1))) return 2;
    const size_t S = (size_t)N - 3, W = (size_t)words_of(N), T = (size_t)table_len(N);
    const int64_t E = (int64_t)R * (int64_t)S;
    std::vector<int32_t> tables((size_t)R * T);
    std::vector<double> lengths((size_t)R * T);
    std::vector<uint8_t> flags((size_t)R);
    if (!read_all(argv[6], tables) || !read_all(argv[7], lengths) || !read_all(argv[8], flags)) return 3;
    // the results, exactly sized, zeroed as the library zeroes them
    int32_t n_splits = -1;
    uint8_t status = 9;
    std::vector<int32_t> count(S, 0), size(S, 0), parent(S, 0), leaf_parent((size_t)N, 0);
    std::vector<double> split_length(S, 0.0), leaf_length((size_t)N, 0.0);
    Args a{};
    a.rep_slots = tables.data(); a.rep_lengths = lengths.data(); a.rep_flag = flags.data();
    a.n_splits = &n_splits; a.count = count.data(); a.size = size.data(); a.parent = parent.data(); a.leaf_parent = leaf_parent.data();
    a.split_length = split_length.data(); a.leaf_length = leaf_length.data(); a.status = &status;
    a.N = N; a.R = R; a.percent = percent; a.b0 = 0; a.nb = 1;
    a.cap = want_cap ? want_cap : capacity_of(E);
    // the state: one exactly sized allocation per array, garbage where no start value is promised
    pfspan::Allocate own;
    state_arrays(own, a, 1, (size_t)R, N, (size_t)a.cap, true);
    std::fill(a.bits, a.bits + (size_t)E * W, 0xdeadbeefdeadbeefull);
    std::fill(a.hash, a.hash + E, 0xdeadbeefdeadbeefull);
    std::fill(a.cbits, a.cbits + S * W, 0xdeadbeefdeadbeefull);
    for (int32_t* p : {a.sizes, a.above, a.low}) std::fill(p, p + E, 12345);
    for (int32_t* p : {a.row, a.leaf_pos}) std::fill(p, p + (size_t)R * (size_t)N, 12345);
    for (int32_t* p : {a.sel, a.order}) std::fill(p, p + S, 12345);
    std::fill(a.slot_of, a.slot_of + E, NONE);
    for (int32_t* p : {a.owner, a.rank_of}) std::fill(p, p + a.cap, NONE);
    std::vector<uint64_t> tile((size_t)TILE * W);

    for (int r = 0; r < R; ++r) splits_group(a, r, threads);
    for (int64_t e = 0; e < E; ++e) keys_entry(a, 0, e);
    // (the counts must not depend on who claims a slot: odd entries first, descending, then the even ones)
    for (int64_t e = E - 1; e >= 0; --e)
        if (e & 1) count_entry(a, PlainTable{}, 0, e);
    for (int64_t e = 0; e < E; ++e)
        if (!(e & 1)) count_entry(a, PlainTable{}, 0, e);
    for (int64_t slot = a.cap - 1; slot >= 0; --slot)
        if (select_slot(a, 0, slot)) select_put(a, PlainTable{}, 0, slot, a.nsel[0]++);
    for (int i = selected_count(a, 0) - 1; i >= 0; --i) rank_selected(a, PlainTable{}, 0, i);
    for (int t0 = 0; t0 < (int)S; t0 += TILE) nest_group(a, t0, threads, tile.data());
    for (int x = 0; x < N; ++x)
        if (!a.err[0]) nest_leaf(a, 0, x);
    for (int64_t e = E - 1; e >= 0; --e) length_entry(a, 0, e);
    for (int u = (int)S + N - 1; u >= 0; --u) finish_thread(a, 0, u);

    FILE* f = fopen(argv[9], "wb");
    if (!f) return 3;
    fwrite(&n_splits, sizeof(int32_t), 1, f);
    fwrite(count.data(), sizeof(int32_t), S, f);
    fwrite(size.data(), sizeof(int32_t), S, f);
    fwrite(parent.data(), sizeof(int32_t), S, f);
    fwrite(leaf_parent.data(), sizeof(int32_t), (size_t)N, f);
    fwrite(split_length.data(), sizeof(double), S, f);
    fwrite(leaf_length.data(), sizeof(double), (size_t)N, f);
    fwrite(&status, 1, 1, f);
    fclose(f);
    printf("clean, N = %d, R = %d, threads = %d, %lld slots, error word %d\n", N, R, threads, (long long)a.cap, a.err[0]);
    return 0;
}
