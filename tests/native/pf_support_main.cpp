// The bodies of the split-support kernels (phyloformer_amd/csrc/pf_support_host.h) run on the CPU in the kernels' own
// geometry - workgroups of `threads` threads, one after the other - with every array allocated at its exact size, for
// AddressSanitizer / UBSan (tests/test_supports_native.py).  One source:
//   pf_support_main N R threads rc tables.bin flags.bin out.bin
// tables.bin: int32 [R + 1][2 (N - 3) + 3], the reference first; flags.bin: uint8 [R]; rc: replicates per chunk.
// out.bin: count int32 [N - 3], transfer int64 [N - 3], depth int32 [N - 3], status uint8.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_support_host.h"

using namespace pfsup;

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(T), v.size(), f);
    fclose(f);
    return got == v.size();
}

// k_sup_splits' workgroup for tree k
static void splits_group(const Args& a, int k, int threads) {
    const int N = a.N, S = N - 3, W = words_of(N);
    if (flagged(a, 0, k)) return;
    const int32_t* slots = slots_of(a, 0, k);
    uint64_t* bits = bits_of(a, 0, k);
    int32_t* row = row_of(a, 0, k);
    for (int tid = 0; tid < threads; ++tid) rows_init(row, N, tid, threads);
    bool ok = true;
    for (int t = 0; t < S && ok; ++t) {
        const int32_t sa = slots[2 * t], sb = slots[2 * t + 1];
        int32_t ra = 0, rb = 0;
        if (!join_ok(PlainRows{row}, N, sa, sb, &ra, &rb)) { ok = false; break; }
        for (int tid = threads - 1; tid >= 0; --tid) join_words(bits, S, W, t, sa, ra, sb, rb, tid, threads);
        row[sa] = t;
        row[sb] = DEAD;
    }
    if (ok) ok = final_ok(PlainRows{row}, N, slots + 2 * (size_t)S);
    if (!ok) { *bad_of(a, 0, k) = 1; return; }
    for (int tid = 0; tid < threads; ++tid) normalise(bits, S, W, N, k == 0 ? a.sizes : nullptr, tid, threads);
}

// k_sup_match's workgroup for (tile, replicate)
static void match_group(const Args& a, int t0, int r, int threads, uint64_t* tile) {
    const int N = a.N, S = N - 3, W = words_of(N);
    int32_t* delta = a.delta + (size_t)r * (size_t)S;
    if (flagged(a, 0, r + 1)) {
        for (int tid = 0; tid < TILE && t0 + tid < S; ++tid) delta[t0 + tid] = delta_of(N, a.sizes[t0 + tid], N);
        return;
    }
    for (int tid = 0; tid < threads; ++tid) tile_load(tile, bits_of(a, 0, 0), S, W, t0, tid, threads);
    int all[TILE];
    for (int k = 0; k < TILE; ++k) all[k] = N;
    for (int tid = 0; tid < threads; ++tid) {
        int best[TILE];
        match_thread(tile, bits_of(a, 0, r + 1), S, W, N, tid, threads, best);
        for (int k = 0; k < TILE; ++k) all[k] = std::min(all[k], best[k]);
    }
    for (int tid = 0; tid < TILE && t0 + tid < S; ++tid) delta[t0 + tid] = delta_of(all[tid], a.sizes[t0 + tid], N);
}

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int N = atoi(argv[1]), R = atoi(argv[2]), threads = atoi(argv[3]), rc = atoi(argv[4]);
    if (N < 4 || R < 1 || threads < 1 || rc < 1) return 2;
    const size_t S = (size_t)N - 3, W = (size_t)words_of(N), T = (size_t)table_len(N);
    std::vector<int32_t> tables((size_t)(R + 1) * T);
    std::vector<uint8_t> flags((size_t)R);
    if (!read_all(argv[5], tables) || !read_all(argv[6], flags)) return 3;
    std::vector<int32_t> count(S, -1), depth(S, -1);
    std::vector<int64_t> transfer(S, -1);
    std::vector<uint8_t> bad((size_t)R + 1, 0);
    uint8_t status = 9;
    for (int r0 = 0; r0 < R; r0 += rc) {
        const int n = std::min(rc, R - r0);
        // a chunk's state, exactly sized and full of garbage
        std::vector<uint64_t> bits((size_t)(n + 1) * S * W, 0xdeadbeefdeadbeefull), tile((size_t)TILE * W);
        std::vector<int32_t> row((size_t)(n + 1) * (size_t)N, 12345), sizes(S, -7), delta((size_t)n * S, -7);
        Args a{};
        a.ref_slots = tables.data(); a.rep_slots = tables.data() + T; a.rep_flag = flags.data();
        a.bits = bits.data(); a.row = row.data(); a.sizes = sizes.data(); a.delta = delta.data(); a.bad = bad.data();
        a.count = count.data(); a.transfer = transfer.data(); a.depth = depth.data(); a.status = &status;
        a.N = N; a.R = R; a.b0 = 0; a.nb = 1; a.r0 = r0; a.rc = n;
        for (int k = 0; k <= n; ++k) splits_group(a, k, threads);
        for (int r = 0; r < n; ++r)
            for (int t0 = 0; t0 < (int)S; t0 += TILE) match_group(a, t0, r, threads, tile.data());
        for (int t = 0; t < (int)S; ++t) sum_split(a, 0, t, r0 == 0);
    }
    FILE* f = fopen(argv[7], "wb");
    if (!f) return 3;
    fwrite(count.data(), sizeof(int32_t), S, f);
    fwrite(transfer.data(), sizeof(int64_t), S, f);
    fwrite(depth.data(), sizeof(int32_t), S, f);
    fwrite(&status, 1, 1, f);
    fclose(f);
    printf("clean, N = %d, R = %d, threads = %d, chunks of %d\n", N, R, threads, rc);
    return 0;
}
