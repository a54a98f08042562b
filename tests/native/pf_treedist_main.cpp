// The bodies of the tree-distance kernels (phyloformer_amd/csrc/pf_treedist_host.h, and pfcon's through it) run on the CPU
// in the kernels' own geometry - workgroups of `threads` threads, one after the other, the entries of the counting kernel
// and the pairs in a scrambled order - with every array allocated at its exact size, for AddressSanitizer / UBSan
// (tests/test_treedist_native.py).  One source:
//   pf_treedist_main N K threads cap tables.bin lengths.bin flags.bin out.bin
// tables.bin: int32 [K][2 (N - 3) + 3]; lengths.bin: double [K][2 (N - 3) + 3]; flags.bin: uint8 [K]; cap: slots of the
// hash table, a power of two (0: the library's).
// out.bin: shared int32 [K][K], kf double [K][K], wrf double [K][K], status uint8.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_treedist_host.h"

using namespace pftd;

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(T), v.size(), f);
    fclose(f);
    return got == v.size();
}

// k_con_splits' workgroup for tree r
static void splits_group(const pfcon::Args& a, int r, int threads) {
    const int N = a.N, S = N - 3, W = words_of(N);
    if (pfcon::flagged(a, 0, r)) return;
    const int32_t* slots = pfcon::slots_of(a, 0, r);
    uint64_t* bits = pfcon::bits_of(a, 0, r);
    const size_t k = pfcon::tree_index(a, 0, r);
    int32_t *row = a.row + k * (size_t)N, *above = a.above + k * (size_t)S, *leaf_pos = a.leaf_pos + k * (size_t)N;
    for (int tid = 0; tid < threads; ++tid) pfsup::rows_init(row, N, tid, threads);
    for (int t = 0; t < S; ++t) {
        const int32_t sa = slots[2 * t], sb = slots[2 * t + 1];
        int32_t ra = 0, rb = 0;
        if (!pfsup::join_ok(pfsup::PlainRows{row}, N, sa, sb, &ra, &rb)) { a.err[0] |= ERR_TABLE; return; }
        for (int tid = threads - 1; tid >= 0; --tid) pfsup::join_words(bits, S, W, t, sa, ra, sb, rb, tid, threads);
        pfcon::branch_at(above, leaf_pos, sa, ra, 2 * t);
        pfcon::branch_at(above, leaf_pos, sb, rb, 2 * t + 1);
        row[sa] = t;
        row[sb] = pfsup::DEAD;
    }
    if (!pfsup::final_ok(pfsup::PlainRows{row}, N, slots + 2 * (size_t)S)) { a.err[0] |= ERR_TABLE; return; }
    for (int tid = 0; tid < 3; ++tid) pfcon::branch_at(above, leaf_pos, slots[2 * S + tid], row[slots[2 * S + tid]], 2 * S + tid);
    for (int tid = 0; tid < threads; ++tid) pfsup::normalise(bits, S, W, N, a.sizes + k * (size_t)S, tid, threads);
}

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    const int N = atoi(argv[1]), K = atoi(argv[2]), threads = atoi(argv[3]);
    const long long want_cap = atoll(argv[4]);
    if (N < 4 || K < 1 || threads < 1 || want_cap < 0 || (want_cap & (want_cap - 1))) return 2;
    const size_t S = (size_t)N - 3, W = (size_t)words_of(N), T = (size_t)table_len(N), k = (size_t)K;
    const int64_t E = (int64_t)K * (int64_t)S;
    std::vector<int32_t> tables(k * T);
    std::vector<double> lengths(k * T);
    std::vector<uint8_t> flags(k);
    if (!read_all(argv[5], tables) || !read_all(argv[6], lengths) || !read_all(argv[7], flags)) return 3;
    // pair_of against the double loop, every pair of this K and the ends of the largest
    {
        int64_t p = 0;
        for (int i = 0; i < K; ++i)
            for (int j = i + 1; j < K; ++j, ++p) {
                int x = -1, y = -1;
                pair_of(p, K, &x, &y);
                if (x != i || y != j) return 4;
            }
        int x = -1, y = -1;
        pair_of(0, MAX_K, &x, &y);
        if (x != 0 || y != 1) return 4;
        pair_of(pairs_of(MAX_K) - 1, MAX_K, &x, &y);
        if (x != MAX_K - 2 || y != MAX_K - 1) return 4;
        for (int i = 0; i < MAX_K - 1; i += 97)
            for (int64_t q : {pair_start(i, MAX_K), pair_start(i + 1, MAX_K) - 1}) {
                pair_of(q, MAX_K, &x, &y);
                if (x != i || y != (int)(q - pair_start(i, MAX_K)) + i + 1) return 4;
            }
    }
    // the results, exactly sized, zeroed as the library zeroes them
    uint8_t status = 9;
    std::vector<int32_t> shared(k * k, 0);
    std::vector<double> kf(k * k, 0.0), wrf(k * k, 0.0);
    Args a{};
    a.c.rep_slots = tables.data(); a.c.rep_lengths = lengths.data(); a.c.rep_flag = flags.data(); a.c.status = &status;
    a.c.N = N; a.c.R = K; a.c.b0 = 0; a.c.nb = 1;
    a.c.cap = want_cap ? want_cap : pfcon::capacity_of(E);
    a.shared = shared.data(); a.kf = kf.data(); a.wrf = wrf.data();
    // the state: one exactly sized allocation per array, garbage where no start value is promised
    pfspan::Allocate own;
    state_arrays(own, a, 1, k, N, (size_t)a.c.cap);
    std::fill(a.c.bits, a.c.bits + (size_t)E * W, 0xdeadbeefdeadbeefull);
    std::fill(a.c.hash, a.c.hash + E, 0xdeadbeefdeadbeefull);
    for (int32_t* p : {a.c.sizes, a.c.above, a.c.low, a.idx_slot, a.idx_entry}) std::fill(p, p + E, 12345);
    for (int32_t* p : {a.c.row, a.c.leaf_pos}) std::fill(p, p + k * (size_t)N, 12345);
    std::fill(a.c.slot_of, a.c.slot_of + E, NONE);
    std::fill(a.c.owner, a.c.owner + a.c.cap, NONE);

    for (int r = 0; r < K; ++r) splits_group(a.c, r, threads);
    for (int64_t e = 0; e < E; ++e) pfcon::keys_entry(a.c, 0, e);
    // (nothing may depend on who claims a slot: odd entries first, descending, then the even ones)
    for (int64_t e = E - 1; e >= 0; --e)
        if (e & 1) pfcon::count_entry(a.c, pfcon::PlainTable{}, 0, e);
    for (int64_t e = 0; e < E; ++e)
        if (!(e & 1)) pfcon::count_entry(a.c, pfcon::PlainTable{}, 0, e);
    for (int64_t e = E - 1; e >= 0; --e) index_entry(a, 0, e);
    for (int64_t p = pairs_of(K) - 1; p >= 0; --p) {
        int i = 0, j = 0;
        pair_of(p, K, &i, &j);
        if (!pair_runs(a, 0, i, j)) continue;
        Acc acc[LANES];
        for (int lane = LANES - 1; lane >= 0; --lane) acc[lane] = pair_lane(a, 0, i, j, lane);
        for (int s = LANES / 2; s > 0; s >>= 1)
            for (int lane = s - 1; lane >= 0; --lane) acc_merge(acc[lane], acc[lane + s]);
        pair_store(a, 0, i, j, acc[0]);
    }
    for (int64_t u = (int64_t)K * K - 1; u >= 0; --u) finish_cell(a, 0, u);

    FILE* f = fopen(argv[8], "wb");
    if (!f) return 3;
    fwrite(shared.data(), sizeof(int32_t), k * k, f);
    fwrite(kf.data(), sizeof(double), k * k, f);
    fwrite(wrf.data(), sizeof(double), k * k, f);
    fwrite(&status, 1, 1, f);
    fclose(f);
    printf("clean, N = %d, K = %d, threads = %d, %lld slots, error word %d\n", N, K, threads, (long long)a.c.cap, a.c.err[0]);
    return 0;
}
