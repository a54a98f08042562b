// Stand-alone walk of the row layout of option "stats_dedup" (csrc/pf_layout.h: row_ctiles, row_ctile_nvalid, row_parts,
// row_part) - the functions k_row_stats calls on the device.  Prints, for every (flat, P, L) asked for, one line per row
// part: "part <flat> <P> <L> <p> <j> <kt> <l0> <slot>", and for every K one line per compact tile: "ctile <K> <ct> <nvalid>";
// tests/test_row_stats_layout.py sets them against a plain Python model.  The program itself checks what needs no model:
// every token of a row sits in exactly one part, in the lane the original tiling gives it; no two parts of an alignment
// share a slot; the slots of a row are consecutive.  Ends with "pf_row_stats_layout_main: clean".
#include <cstdio>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_layout.h"

using namespace pfk;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void walk(int flat, int P, int L, bool print) {
    const int nt_aln = flat ? (int)(((long)P * L + 31) / 32) : P * ((L + 31) / 32);
    const int slots_aln = flat ? nt_aln + P : nt_aln;
    std::vector<int> slot_used((size_t)slots_aln, 0);
    for (int p = 0; p < P; ++p) {
        std::vector<int> seen((size_t)L, 0);
        const int n = row_parts(flat, L, p);
        CHECK(n >= 1, "flat %d P %d L %d row %d: %d parts", flat, P, L, p, n);
        int prev_slot = -1;
        for (int j = 0; j < n; ++j) {
            const RowPart r = row_part(flat, L, p, j);
            if (print) std::printf("part %d %d %d %d %d %d %d %d\n", flat, P, L, p, j, r.kt, r.l0, r.slot);
            CHECK(r.kt >= 0 && r.kt < nt_aln && r.slot >= 0 && r.slot < slots_aln, "flat %d P %d L %d row %d part %d: tile %d slot %d", flat, P, L, p, j, r.kt, r.slot);
            if (r.slot < 0 || r.slot >= slots_aln) continue;
            slot_used[(size_t)r.slot]++;
            CHECK(j == 0 || r.slot == prev_slot + 1, "flat %d P %d L %d row %d part %d: slot %d behind %d", flat, P, L, p, j, r.slot, prev_slot);
            prev_slot = r.slot;
            int valid = 0;
            for (int t = 0; t < 32; ++t) {
                const int l = r.l0 + t;
                if (l < 0 || l >= L) continue;
                ++valid;
                seen[(size_t)l]++;
                // the lane the original tiling gives token (p, l): flat, token p L + l of the alignment sits in tile
                // (p L + l) / 32 at lane (p L + l) % 32; by rows, in tile p ntiles + l / 32 at lane l % 32
                const long tok = flat ? (long)p * L + l : (long)p * ((L + 31) / 32) * 32 + l;
                CHECK(tok / 32 == r.kt && tok % 32 == t, "flat %d P %d L %d token (%d, %d): tile %d lane %d", flat, P, L, p, l, r.kt, t);
            }
            CHECK(valid >= 1, "flat %d P %d L %d row %d part %d holds no token", flat, P, L, p, j);
        }
        for (int l = 0; l < L; ++l) CHECK(seen[(size_t)l] == 1, "flat %d P %d L %d: token (%d, %d) in %d parts", flat, P, L, p, l, seen[(size_t)l]);
    }
    for (int s = 0; s < slots_aln; ++s)
        CHECK(slot_used[(size_t)s] <= 1, "flat %d P %d L %d: slot %d used %d times", flat, P, L, s, slot_used[(size_t)s]);
}

int main() {
    for (int P = 1; P <= 6; ++P)
        for (int L = 1; L <= 100; ++L) {
            walk(0, P, L, true);
            if (L >= 32 && L % 32 != 0) walk(1, P, L, true);        // the flat tiling's domain (tile_plan_core)
        }
    walk(0, 1770, 500, false);
    walk(1, 1770, 500, false);
    for (int K = 1; K <= 100; ++K) {
        int covered = 0;
        for (int ct = 0; ct < row_ctiles(K); ++ct) {
            const int nv = row_ctile_nvalid(K, ct);
            std::printf("ctile %d %d %d\n", K, ct, nv);
            CHECK(nv >= 1 && nv <= 32 && (nv == 32 || ct == row_ctiles(K) - 1), "K %d tile %d: %d tokens", K, ct, nv);
            covered += nv;
        }
        CHECK(covered == K, "K %d: %d tokens covered", K, covered);
    }
    CHECK(ROW_STATS_KMAX >= 425 && ROW_STATS_KMAX >= 406, "KMAX %d", ROW_STATS_KMAX);       // 17 / 20 of 500; the bench data's largest
    CHECK(ROW_STATS_LDS_BYTES <= 160 * 1024 && ROW_STATS_LDS_BYTES + ROW_STATS_TERM * 4 > 160 * 1024, "LDS %d", ROW_STATS_LDS_BYTES);
    std::printf("kmax %d\n", ROW_STATS_KMAX);
    if (fails) { std::printf("pf_row_stats_layout_main: %d failures\n", fails); return 1; }
    std::printf("pf_row_stats_layout_main: clean\n");
    return 0;
}
