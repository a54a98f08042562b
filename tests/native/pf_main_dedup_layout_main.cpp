// Stand-alone walk of the compact tiling of option "main_dedup" (csrc/pf_layout.h: compact_tiles, compact_tile,
// compact_next, main_dedup_split) - the functions k_main's compact launch and k_main_plan call on the device.
// For every small (P, K): every compacted token (row, u) is covered exactly once, a tile covers at most two rows, only
// the alignment's last tile is ragged (K >= 32; below that one tile of K tokens per row), and stepping with
// compact_next gives what compact_tile computes from the tile number.  Prints "pf_main_dedup_layout_main: clean".
#include <cstdio>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_layout.h"

using namespace pfk;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void walk(int P, int K) {
    const int nt = compact_tiles(P, K);
    std::vector<int> seen((size_t)P * K, 0);
    int r0 = 0, u0 = 0;
    for (int kt = 0; kt < nt; ++kt) {
        const CompactTile c = compact_tile(P, K, kt);
        CHECK(c.r0 == r0 && c.u0 == u0, "P %d K %d tile %d: (%d, %d) by number, (%d, %d) by stepping", P, K, kt, c.r0, c.u0, r0, u0);
        CHECK(c.nvalid >= 1 && c.nvalid <= 32, "P %d K %d tile %d: %d tokens", P, K, kt, c.nvalid);
        CHECK(c.nvalid == compact_nvalid(P, K, kt) && c.wrap == compact_wrap(P, K, c.r0, c.u0), "P %d K %d tile %d", P, K, kt);
        if (K >= 32) CHECK(c.nvalid == 32 || kt == nt - 1, "P %d K %d tile %d of %d is ragged (%d)", P, K, kt, nt, c.nvalid);
        else CHECK(c.nvalid == K && c.wrap == 32, "P %d K %d tile %d: %d tokens, wrap %d", P, K, kt, c.nvalid, c.wrap);
        int first_row = -1, last_row = -1;
        for (int t = 0; t < c.nvalid; ++t) {                  // the lanes, as k_main's lane_pos places them
            const bool in_r1 = t >= c.wrap;
            const int row = c.r0 + (in_r1 ? 1 : 0), u = c.u0 + t - (in_r1 ? K : 0);
            CHECK(row >= 0 && row < P && u >= 0 && u < K, "P %d K %d tile %d lane %d: (%d, %d)", P, K, kt, t, row, u);
            if (row < 0 || row >= P || u < 0 || u >= K) continue;
            seen[(size_t)row * K + u]++;
            if (first_row < 0) first_row = row;
            last_row = row;
        }
        CHECK(last_row - first_row <= 1, "P %d K %d tile %d covers rows %d..%d", P, K, kt, first_row, last_row);
        CHECK((c.wrap < 32) == (last_row != first_row), "P %d K %d tile %d: wrap %d, rows %d..%d", P, K, kt, c.wrap, first_row, last_row);
        compact_next(K, &r0, &u0);
    }
    for (size_t i = 0; i < seen.size(); ++i)
        CHECK(seen[i] == 1, "P %d K %d: token (%d, %d) covered %d times", P, K, (int)(i / K), (int)(i % K), seen[i]);
}

int main() {
    for (int P = 1; P <= 12; ++P)
        for (int K = 1; K <= 130; ++K) walk(P, K);
    walk(1770, 182);
    walk(1770, 497);
    // the routes: 0 never, 2 always, 1 by the alignment's own share of distinct columns, monotone in K
    for (int L = 1; L <= 600; L += 7) {
        bool prev = true;
        for (int K = 1; K <= L; ++K) {
            CHECK(!main_dedup_split(K, L, 0) && main_dedup_split(K, L, 2), "L %d K %d", L, K);
            const bool s = main_dedup_split(K, L, 1);
            CHECK(prev || !s, "L %d K %d: split above a fused count", L, K);
            CHECK(s == ((long)K * MAIN_DEDUP_DEN <= (long)L * MAIN_DEDUP_NUM), "L %d K %d", L, K);
            prev = s;
        }
        CHECK(compact_tiles(3, L) <= (3 * L + 31) / 32 || L < 32, "L %d", L);
    }
    CHECK(main_plan_ints(16) == 4 + 3 * 16 + 1, "plan size");
    if (fails) { std::printf("pf_main_dedup_layout_main: %d failures\n", fails); return 1; }
    std::printf("pf_main_dedup_layout_main: clean\n");
    return 0;
}
