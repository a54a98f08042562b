// The bodies of the transfer-count kernels (phyloformer_amd/csrc/pf_support_host.h: the matching that keeps its key,
// k_sup_moves) run on the CPU in the kernels' own geometry - workgroups of `threads` threads, one after the other - with
// every array allocated at its exact size, for AddressSanitizer / UBSan (tests/test_transfers_native.py).  One source:
//   pf_transfers_main N R threads rc cutoff branch tables.bin flags.bin out.bin
// tables.bin: int32 [R + 1][2 (N - 3) + 3], the reference first; flags.bin: uint8 [R]; rc: replicates per chunk; branch:
// 1 with branch_moves, 0 without.
// out.bin: count int32 [S], transfer int64 [S], depth int32 [S], moves int64 [N], used int32 [S], capped int32 [S],
// branch_moves int32 [S][N] (with branch), status uint8; S = N - 3.
// The staging list of pf_join_transfers is carved for (B, R) = (3, 2) on the way: every array aligned for its type, no
// two overlapping, the whole as long as measured.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
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

// k_sup_match<true>'s workgroup for (tile, replicate): the threads' keys meet in descending order of the thread
static void match_group(const Args& a, const Transfers& x, int t0, int r, int threads, uint64_t* tile) {
    const int N = a.N, S = N - 3, W = words_of(N);
    int32_t* delta = a.delta + (size_t)r * (size_t)S;
    int32_t* arg = x.arg + (size_t)r * (size_t)S;
    if (flagged(a, 0, r + 1)) {
        for (int tid = 0; tid < TILE && t0 + tid < S; ++tid) {
            delta[t0 + tid] = delta_of(N, a.sizes[t0 + tid], N);
            arg[t0 + tid] = key_none(N);
        }
        return;
    }
    for (int tid = 0; tid < threads; ++tid) tile_load(tile, bits_of(a, 0, 0), S, W, t0, tid, threads);
    int all[TILE];
    for (int k = 0; k < TILE; ++k) all[k] = key_none(N);
    for (int tid = threads - 1; tid >= 0; --tid) {
        int best[TILE];
        match_thread<true>(tile, bits_of(a, 0, r + 1), S, W, N, tid, threads, best);
        for (int k = 0; k < TILE; ++k) all[k] = std::min(all[k], best[k]);
    }
    for (int tid = 0; tid < TILE && t0 + tid < S; ++tid) {
        delta[t0 + tid] = delta_of(key_m(all[tid]), a.sizes[t0 + tid], N);
        arg[t0 + tid] = all[tid];
    }
}

// a visitor of the staging list: the spans as Carve lays them out
struct Spans {
    pfspan::Carve c;
    std::vector<std::pair<size_t, size_t>> spans;      // (offset, bytes)
    bool aligned = true;
    template <class T> void operator()(T*& p, size_t count) {
        const char* before = c.at;
        c(p, count);
        aligned = aligned && reinterpret_cast<uintptr_t>(p) % alignof(T) == 0;
        spans.push_back({(size_t)reinterpret_cast<uintptr_t>(before), count * sizeof(T)});
    }
};

static bool staging_ok(int N) {
    for (int branch = 0; branch < 2; ++branch) {
        TransferStaging io{};
        const size_t B = 3, R = 2;
        auto list = [&](auto& v) { transfer_staging_arrays(v, io, B, R, N, branch != 0); };
        const size_t bytes = pfspan::measure(list);
        std::vector<uint64_t> block(bytes / 8 + 1);
        char* base = reinterpret_cast<char*>(block.data());
        Spans v{pfspan::Carve{base}, {}, true};
        list(v);
        if (!v.aligned || (size_t)(v.c.at - base) != bytes || v.spans.size() != 11) return false;
        for (size_t i = 0; i + 1 < v.spans.size(); ++i)
            if (v.spans[i].first + v.spans[i].second > v.spans[i + 1].first) return false;
        const size_t S = (size_t)N - 3;
        if (v.spans[7].second != B * (size_t)N * sizeof(int64_t) || v.spans[8].second != B * S * sizeof(int32_t) ||
            v.spans[10].second != (branch ? B * S * (size_t)N * sizeof(int32_t) : 0))
            return false;
        // every byte of every array can be written
        std::fill(io.moves, io.moves + B * (size_t)N, (int64_t)-1);
        std::fill(io.used, io.used + B * S, -1);
        std::fill(io.capped, io.capped + B * S, -1);
        if (branch) std::fill(io.branch, io.branch + B * S * (size_t)N, -1);
        std::fill(io.status, io.status + B, (uint8_t)1);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int N = atoi(argv[1]), R = atoi(argv[2]), threads = atoi(argv[3]), rc = atoi(argv[4]), cutoff = atoi(argv[5]);
    const bool branch = atoi(argv[6]) != 0;
    if (N < 4 || R < 1 || threads < 1 || rc < 1 || cutoff < 0 || cutoff > 100) return 2;
    if (!staging_ok(N)) return 4;
    const size_t S = (size_t)N - 3, W = (size_t)words_of(N), T = (size_t)table_len(N);
    std::vector<int32_t> tables((size_t)(R + 1) * T);
    std::vector<uint8_t> flags((size_t)R);
    if (!read_all(argv[7], tables) || !read_all(argv[8], flags)) return 3;
    std::vector<int32_t> count(S, -1), depth(S, -1), used(S, -1), capped(S, -1), rows(branch ? S * (size_t)N : 0, -1);
    std::vector<int64_t> transfer(S, -1), moves((size_t)N, -1);
    std::vector<uint8_t> bad((size_t)R + 1, 0);
    uint8_t status = 9;
    for (int r0 = 0; r0 < R; r0 += rc) {
        const int n = std::min(rc, R - r0);
        const bool first = r0 == 0;
        // a chunk's state, exactly sized and full of garbage
        std::vector<uint64_t> bits((size_t)(n + 1) * S * W, 0xdeadbeefdeadbeefull), tile((size_t)TILE * W);
        std::vector<int32_t> row((size_t)(n + 1) * (size_t)N, 12345), sizes(S, -7), delta((size_t)n * S, -7), arg((size_t)n * S, -7);
        Args a{};
        a.ref_slots = tables.data(); a.rep_slots = tables.data() + T; a.rep_flag = flags.data();
        a.bits = bits.data(); a.row = row.data(); a.sizes = sizes.data(); a.delta = delta.data(); a.bad = bad.data();
        a.count = count.data(); a.transfer = transfer.data(); a.depth = depth.data(); a.status = &status;
        a.N = N; a.R = R; a.b0 = 0; a.nb = 1; a.r0 = r0; a.rc = n;
        const Transfers x{arg.data(), moves.data(), used.data(), capped.data(), branch ? rows.data() : nullptr, cutoff};
        for (int k = 0; k <= n; ++k) splits_group(a, k, threads);
        for (int r = 0; r < n; ++r)
            for (int t0 = 0; t0 < (int)S; t0 += TILE) match_group(a, x, t0, r, threads, tile.data());
        for (int t = 0; t < (int)S; ++t) sum_split(a, 0, t, first);
        if (first) std::fill(moves.begin(), moves.end(), 0);        // (the launch's memset)
        // k_sup_moves' workgroups, the last split first: the sums into moves come in another order than the twin's
        for (int t = (int)S - 1; t >= 0; --t)
            for (int tid = threads - 1; tid >= 0; --tid) moves_thread(a, x, 0, t, first, tid, threads, PlainKeys{}, PlainAdd{});
    }
    FILE* f = fopen(argv[9], "wb");
    if (!f) return 3;
    fwrite(count.data(), sizeof(int32_t), S, f);
    fwrite(transfer.data(), sizeof(int64_t), S, f);
    fwrite(depth.data(), sizeof(int32_t), S, f);
    fwrite(moves.data(), sizeof(int64_t), (size_t)N, f);
    fwrite(used.data(), sizeof(int32_t), S, f);
    fwrite(capped.data(), sizeof(int32_t), S, f);
    if (branch) fwrite(rows.data(), sizeof(int32_t), rows.size(), f);
    fwrite(&status, 1, 1, f);
    fclose(f);
    printf("clean, N = %d, R = %d, threads = %d, chunks of %d, cutoff %d\n", N, R, threads, rc, cutoff);
    return 0;
}
