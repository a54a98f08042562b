// Shapes and memory-layout constants shared by the device kernels (pf_device.hip.h) and the host-side weight
// preparation (pf_host_prep.h).  Plain C++: no HIP types, so that the host code builds with g++ under
// AddressSanitizer / UBSan for the fuzz tests (tests/test_native_sanitizers.py).
#pragma once

// 16-bit format of the split MFMA operands: 1 = IEEE half (default), 0 = bfloat16 (rounds 1-5; A/B builds only).
// pf_device.hip.h explains the choice; pf_host_prep.h packs the weights accordingly.
#ifndef PF_F16
#define PF_F16 1
#endif

namespace pfk {

constexpr int E = 64;        // embed_dim
constexpr int NH = 4;        // heads
constexpr int HD = 16;       // head_dim
constexpr int FF = 256;      // FFN hidden
constexpr int NA = 22;       // alphabet
constexpr int SROW = 72;     // row statistics per pair
constexpr int MROW = 4 * 64; // folded row mix per pair: M[h][c], 4 heads (the bias row is the same for every pair:
                             // k_colstats keeps it in registers, the MFMA fragments carry it in K slot 4)
constexpr float LN_EPS = 1e-5f;

// LDS image of one block's MFMA A operands (fragments of 8 16-bit values, 16 B per lane):
//   W1' : [8 T][4 s][2 hi/lo][64 lanes]      64 KB   (FFN 64->256, LN affine folded)
//   W2  : [2 To][16 s][2][64]                64 KB   (FFN 256->64)
//   Woc : [2 To][4 s][2][64]                 16 KB   (column out_proj)
//   Wv' : [2 T][4 s][64] hi only              8 KB   (next block's row V projection; lo: below / L2)
//   Wqk : [4 s][2][16]                         2 KB   (next block's row q/k rows, 8 of 32 rows)
//   Wv' lo : [WVLO_LDS of 2 T x 4 s][64]       4 KB   (the first four of the eight lo fragments; the rest from L2)
//   consts (floats): b1'[256] | b2[64] | bqk[8] | head_w[64] | head_b[1] | c0[1] | pad | bo_col[64]
// The last block has no next row attention: its [FRAG_WV, FRAG_END) tail holds the folded head instead (FRAG_U),
// u = W2^T head_w as fp32 in lane order [8 T][2 h][16 r] (hidden row 32 T + kmap(r, h), the row GEMM1's accumulator
// register r holds), and c0 = head_w . b2 + head_b (pf_host_prep.h, fold_head; k_main<MODE_LAST_FOLD>).
constexpr int FRAG_W1 = 0;                                   // [8 T][4 s][2 hi/lo][64]
constexpr int FRAG_W2 = FRAG_W1 + 8 * 4 * 2 * 64;            // [2 To][16 s][2][64]
constexpr int FRAG_WO = FRAG_W2 + 2 * 16 * 2 * 64;           // [2 To][4 s][2][64]
constexpr int FRAG_WV = FRAG_WO + 2 * 4 * 2 * 64;            // next row attn Wv' hi only: [2 T][4 s][64]
constexpr int FRAG_QK = FRAG_WV + 2 * 4 * 64;                // next row attn [Wq';Wk'] rows 0..7 only:
                                                             //   [4 s][2 hi/lo][2 kgrp][8 rows]
#ifndef PF_WVLO_LDS
#define PF_WVLO_LDS 4        // of the 8 Wv' lo fragments per lane, how many live in LDS (what fits: 4 KB of the 4,288 B left)
#endif
constexpr int WVLO_LDS = PF_WVLO_LDS;
constexpr int FRAG_WVLO = FRAG_QK + 4 * 2 * 16;              // the first WVLO_LDS of Wv' lo's [2 T][4 s] fragments: [..][64]
constexpr int FRAG_END = FRAG_WVLO + WVLO_LDS * 64;          // in fragment (16-byte) units
constexpr int FRAG_U = FRAG_WV;                              // last block only: u[8 T][2 h][16 r] fp32 (1 KB)
constexpr int U_FRAGS = FF * 4 / 16;
static_assert(FRAG_U + U_FRAGS <= FRAG_END, "the folded head fits the last block's tail");
constexpr int WVLO_FRAGS = 2 * 4 * 64;                       // lo part of Wv', read from global
constexpr int CONST_B1 = 0, CONST_B2 = 256, CONST_BQK = 320, CONST_HW = 328, CONST_HB = 392,
              CONST_C0 = 393, CONST_BOC = 400;
constexpr int CONST_LEN = 464;                                // floats
constexpr int MAIN_LDS_BYTES = FRAG_END * 16 + CONST_LEN * 4; // 163,648 B of the 163,840 B LDS (159,552 without Wv' lo)
constexpr int MFRAG_PER_PAIR = 2 * 2 * 32;                    // row-mix fragments per pair (lanes h=0)

constexpr int MAIN_THREADS = 512;  // 8 waves: two per SIMD so MFMA and VALU phases of different waves overlap
constexpr int MAIN_WAVES = MAIN_THREADS / 64;

constexpr int PAIRTAB_ROWS = 22 * 22, PAIRTAB_W = 72;

// ---- option "main_dedup": the compacted tokens of an alignment and their tiles ----------------------------------
// An alignment with K distinct columns of L (k_site_classes) has P x K compacted tokens (row p, u), u < K, token u of a
// row standing at site ulist[u].  k_main's compact launch cuts them into tiles of 32 the way the flat tiling cuts the
// P x L tokens: 32 CONSECUTIVE compacted tokens per tile, a tile may end row r0 and start row r0 + 1 (K >= 32: never
// more than two rows), only the alignment's last tile is ragged.  K < 32: one ragged tile per row, as the row tiling
// has it.  Shared by the kernels and the host (tests/test_main_dedup_layout.py walks it on the CPU).
#if defined(__HIPCC__)
#define PF_HD __host__ __device__
#else
#define PF_HD
#endif
// An alignment takes the split route (compact launch + statistics launch) iff K * DEN <= L * NUM; mode 0: never,
// mode 2: always (tests).  NUM / DEN is the measured break-even of K / L (DESIGN.md section 9,
// profiles/main_dedup_threshold.txt).
#ifndef PF_MAIN_DEDUP_NUM
#define PF_MAIN_DEDUP_NUM 17         // (A/B builds: tools/build_variant.py lib_x.so -DPF_MAIN_DEDUP_NUM=.. -DPF_MAIN_DEDUP_DEN=..)
#define PF_MAIN_DEDUP_DEN 20
#endif
constexpr int MAIN_DEDUP_NUM = PF_MAIN_DEDUP_NUM, MAIN_DEDUP_DEN = PF_MAIN_DEDUP_DEN;
PF_HD inline bool main_dedup_split(int K, int L, int mode) {
    return mode == 2 || (mode == 1 && (long)K * MAIN_DEDUP_DEN <= (long)L * MAIN_DEDUP_NUM);
}
// the most distinct columns an alignment of L sites on the split route can have
PF_HD inline int main_dedup_max_k(int L, int mode) {
    return mode == 2 ? L : mode == 1 ? (int)((long)L * MAIN_DEDUP_NUM / MAIN_DEDUP_DEN) : 0;
}
PF_HD inline int compact_tiles(int P, int K) { return K >= 32 ? (int)(((long)P * K + 31) >> 5) : P; }
// tokens of tile kt (1..32), and the lane from which a tile at (r0, u0) belongs to row r0 + 1 (32: none)
PF_HD inline int compact_nvalid(int P, int K, int kt) {
    const long left = K >= 32 ? (long)P * K - (long)kt * 32 : K;
    return left < 32 ? (int)left : 32;
}
PF_HD inline int compact_wrap(int P, int K, int r0, int u0) {
    return (K >= 32 && r0 + 1 < P && K - u0 < 32) ? K - u0 : 32;
}
struct CompactTile { int r0, u0, nvalid, wrap; };   // row and compacted index of the first token; see above
PF_HD inline CompactTile compact_tile(int P, int K, int kt) {
    CompactTile c;
    if (K >= 32) { const long tok0 = (long)kt * 32; c.r0 = (int)(tok0 / K); c.u0 = (int)(tok0 - (long)c.r0 * K); }
    else { c.r0 = kt; c.u0 = 0; }
    c.nvalid = compact_nvalid(P, K, kt);
    c.wrap = compact_wrap(P, K, c.r0, c.u0);
    return c;
}
// the tile that follows tile (r0, u0) of the same alignment
PF_HD inline void compact_next(int K, int* r0, int* u0) {
    if (K < 32) { ++*r0; return; }
    *u0 += 32;
    if (*u0 >= K) { *u0 -= K; ++*r0; }
}
// The plan k_main_plan writes per run of B alignments (ints): [0] fused alignments nf, [1] split alignments ns,
// [2] compact tiles of all split alignments, [3] unused | flist [B] | slist [B] | cpre [B + 1] (tiles in front of
// split alignment i; cpre[ns] = the total)
PF_HD inline int main_plan_ints(int B) { return 4 + 3 * B + 1; }

// ---- option "stats_dedup": the split route's row statistics per pair row (k_row_stats) ---------------------------
// One work item is a pair row p of a split-route alignment with K <= ROW_STATS_KMAX distinct columns.  Phase 1 forms,
// once per distinct column, what a token gives the statistics before any positional step - v (64), q' (4), k' (4) -
// over the row's COMPACT tiles (32 consecutive entries of ulist, the last one ragged) and keeps it in an LDS term table;
// phase 2 walks the row's PARTS of the original tiling (flat or by rows) and reduces the terms of every site in place.
// LDS of the kernel: Wv' hi | Wq'k' | Wv' lo (all eight fragments) | bqk | site -> compact index | term table.
constexpr int ROW_STATS_FRAG_WV = 0;                                   // [2 T][4 s][64]
constexpr int ROW_STATS_FRAG_QK = ROW_STATS_FRAG_WV + 2 * 4 * 64;      // [4 s][2 hi/lo][2 kgrp][8 rows]
constexpr int ROW_STATS_FRAG_WVLO = ROW_STATS_FRAG_QK + 4 * 2 * 16;    // [2 T][4 s][64]
constexpr int ROW_STATS_FRAGS = ROW_STATS_FRAG_WVLO + WVLO_FRAGS;
constexpr int ROW_STATS_MAP_SITES = 4096;    // sites the map holds (k_site_classes finds no classes beyond: K = L there)
// a token's terms: [2 h][32] v in the lanes' register order | q' [4] | k' [4], padded from 72 to 76 floats: 19 x 16 bytes,
// an odd count, so that sixteen lanes reading consecutive terms with ds_read_b128 meet sixteen different bank groups
constexpr int ROW_STATS_TERM = 76;
constexpr int ROW_STATS_OFF_BQK = ROW_STATS_FRAGS * 16;
constexpr int ROW_STATS_OFF_MAP = ROW_STATS_OFF_BQK + 8 * 4;
constexpr int ROW_STATS_OFF_TERM = ROW_STATS_OFF_MAP + ROW_STATS_MAP_SITES * 2;
constexpr int ROW_STATS_KMAX = 451;          // what the 160 KB leave (a literal: the tests read it out of this line)
static_assert(ROW_STATS_KMAX == (160 * 1024 - ROW_STATS_OFF_TERM) / (ROW_STATS_TERM * 4), "KMAX is derived from the LDS left");
constexpr int ROW_STATS_LDS_BYTES = ROW_STATS_OFF_TERM + ROW_STATS_KMAX * ROW_STATS_TERM * 4;
static_assert(ROW_STATS_KMAX >= 425, "every split-route alignment of 500 sites (K <= 17 / 20 L) fits the term table");
static_assert(ROW_STATS_OFF_TERM % 16 == 0 && ROW_STATS_LDS_BYTES <= 160 * 1024, "the term table is read 16 bytes at a time");
// compact tiles of a row and the tokens of tile ct (compacted tokens 32 ct .. of the row)
PF_HD inline int row_ctiles(int K) { return (K + 31) >> 5; }
PF_HD inline int row_ctile_nvalid(int K, int ct) { return K - 32 * ct < 32 ? K - 32 * ct : 32; }
// Part j of row p in the original tiling: tile kt of the alignment, lane t holds site l0 + t of the row (a token of the
// part iff 0 <= l0 + t < L: l0 < 0 where a flat tile starts in row p - 1), partial slot `slot` of the alignment
// (pf_device.hip.h, part_range: kt + p flat, kt by rows).
struct RowPart { int kt, l0, slot; };
PF_HD inline int row_parts(int flat, int L, int p) {
    if (!flat) return (L + 31) >> 5;
    return (int)(((((long)p + 1) * L - 1) >> 5) - (((long)p * L) >> 5)) + 1;
}
PF_HD inline RowPart row_part(int flat, int L, int p, int j) {
    RowPart r;
    if (!flat) { r.kt = p * ((L + 31) >> 5) + j; r.l0 = 32 * j; r.slot = r.kt; return r; }
    r.kt = (int)(((long)p * L) >> 5) + j;
    r.l0 = (int)((long)r.kt * 32 - (long)p * L);
    r.slot = r.kt + p;
    return r;
}

}  // namespace pfk
