// The taxon axis of derived alignments (pf_gather_taxa_device, pf_forward_taxa, pf_forward_leave_one_out,
// pf_loo_stats_device): k_gather_taxa builds row subsets in HBM from one upload of the source alignments, k_loo_taxon
// and k_loo_pair reduce the distances of the N leave-one-out cuts of an alignment against those of the whole.
//
// k_gather_taxa   src uint8 [B][N][L] -> dst uint8 [B][S][M][L]: row m of set s of every source is source row
//                 taxa[s][m] (device int32 [..][M]; any rows of [0, N): repeats, any order, M may exceed N;
//                 phyloformer_amd/taxa.py::cut_taxa is the host twin).  The work split is k_gather_sites': one
//                 workgroup per (tile of GT_TILE sites, set), a thread copies runs of 4 consecutive sites of one row,
//                 consecutive threads take consecutive runs of a row.  Neither a source row (b N + t) L nor a
//                 destination row is 4-byte aligned in general, so a row's tile is cut at the DESTINATION's dword
//                 boundaries: a head of 0..3 bytes (item 0 of the row), whole dwords - one 32-bit store each, their four
//                 source bytes read by load_run4 with the widest loads the source address allows - and a tail of
//                 0..3 bytes, heads and tails through byte stores.
//                 A table that only ever existed on the device cannot be validated up front: an entry outside [0, N)
//                 is never dereferenced (row 0 is read in its place) and raises the sticky flag `bad`, which the next
//                 pf_synchronize / pf_memcpy_d2h reports as PF_EINVAL.
//
// Leave-one-out statistics (phyloformer_amd/taxa.py::loo_stats is the host twin).  full float [B][P], P = N (N - 1) / 2
// in the reference's pair order; loo float [B][N][P1], P1 = (N - 1)(N - 2) / 2, set t = the alignment without row t.
// With delta_t(i, j) = loo[t][loo_pair_index(i, j, t, N)] - full[pair_index(i, j, N)] (exact in double):
//
//   influence[b][t]    = sqrt( mean over the P1 pairs of delta_t^2 )           how far removing t moves the others
//   shift[b][t]        = mean over the P1 pairs of delta_t                     signed
//   context[b][(i,j)]  = sqrt( sum_{t != i, j} delta_t(i, j)^2 / (N - 2) )     how much the distance depends on the rest
//
// Accumulated in double, rounded to float once, no atomics: the bits are a function of (N, values) only.
//   k_loo_taxon   one wave per (b, t): lane l adds the pairs l, l + 64, ... of set t in that order (coalesced along the
//                 set), the 64 lane sums meet in a fixed xor tree.
//   k_loo_pair    one thread per (b, pair): adds t = 0 .. N - 1 in index order (for one t, neighbouring pairs of a row
//                 read neighbouring floats of set t).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_bytes.hip.h"
#include "pf_taxa_host.h"

namespace pft {

constexpr int GT_THREADS = 256;
constexpr int GT_TILE = 1024;          // sites per workgroup
constexpr int GT_MAX_Y = 65535;        // sets per launch (grid y)
constexpr int LT_WAVES = 4;            // (b, t) rows per workgroup of k_loo_taxon
constexpr int LP_THREADS = 256;        // pairs per workgroup of k_loo_pair

struct GatherTaxaArgs {
    const uint8_t* src;    // [B][N][L]
    uint8_t* dst;          // [B][S][M][L]
    const int32_t* taxa;   // [..][M], row s_begin + s for dst's set s
    unsigned* bad;         // host-mapped sticky flag: a table entry out of range was seen (may be null)
    int B, N, L, M;
    int s_begin;           // table row of dst's set 0
    int S;                 // sets in dst
    int s_first;           // dst set of this launch's blockIdx.y = 0
};

// grid (ceil(L / GT_TILE), sets of this launch), block GT_THREADS
__global__ __launch_bounds__(GT_THREADS) void k_gather_taxa(GatherTaxaArgs a) {
    const int l0 = blockIdx.x * GT_TILE;
    const int nl = min(GT_TILE, a.L - l0);
    const int sl = a.s_first + (int)blockIdx.y;                        // set in dst
    const int32_t* tab = a.taxa + (size_t)(a.s_begin + sl) * (size_t)a.M;
    const int runs = 1 + (nl + 3) / 4;                                 // the head, then dwords of the destination
    const size_t rows = (size_t)a.B * a.M, L = (size_t)a.L;
    const size_t items = rows * (size_t)runs;
    for (size_t it = threadIdx.x; it < items; it += GT_THREADS) {
        const size_t row = it / (size_t)runs;                          // b * M + m
        const int r = (int)(it - row * (size_t)runs);
        const size_t b = row / (size_t)a.M, m = row - b * (size_t)a.M;
        int t = tab[m];
        if ((unsigned)t >= (unsigned)a.N) {                            // (never taken on a validated table)
            if (a.bad) *a.bad = 1u;
            t = 0;
        }
        const uint8_t* s = a.src + (b * (size_t)a.N + (size_t)t) * L + (size_t)l0;
        uint8_t* d = a.dst + ((b * (size_t)a.S + (size_t)sl) * (size_t)a.M + m) * L + (size_t)l0;
        const int head = min(nl, (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 3u)) & 3u));
        if (r == 0) {
            for (int j = 0; j < head; ++j) d[j] = s[j];
            continue;
        }
        const int k = head + 4 * (r - 1);
        const int len = min(4, nl - k);
        if (len == 4) {
            *reinterpret_cast<uint32_t*>(d + k) = pfbytes::load_run4(s + k);
        } else {
            for (int j = 0; j < len; ++j) d[k + j] = s[k + j];         // (len <= 0: this row had a longer head)
        }
    }
}

// Asynchronous on `s`: rows s_begin .. s_begin + S - 1 of the table into dst [B][S][M][L], in launches of at most
// GT_MAX_Y sets.
inline hipError_t launch_gather_taxa(hipStream_t s, const uint8_t* src, int B, int N, int L, const int32_t* taxa, int s_begin,
                                     int S, int M, uint8_t* dst, unsigned* bad) {
    GatherTaxaArgs a{src, dst, taxa, bad, B, N, L, M, s_begin, S, 0};
    const unsigned tiles = (unsigned)((L + GT_TILE - 1) / GT_TILE);
    for (int s0 = 0; s0 < S; s0 += GT_MAX_Y) {
        a.s_first = s0;
        hipLaunchKernelGGL(k_gather_taxa, dim3(tiles, (unsigned)std::min(GT_MAX_Y, S - s0)), dim3(GT_THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// grid ceil(rows / LT_WAVES), block 64 * LT_WAVES; rows = B * N
__global__ __launch_bounds__(64 * LT_WAVES) void k_loo_taxon(const float* full, const float* loo, float* influence, float* shift,
                                                            size_t rows, int N) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * LT_WAVES + (threadIdx.x >> 6);      // b * N + t
    if (row >= rows) return;                                                    // (wave-uniform)
    const size_t b = row / (size_t)N;
    const int t = (int)(row - b * (size_t)N);
    const int P = N * (N - 1) / 2, P1 = (N - 1) * (N - 2) / 2;
    const float* f = full + b * (size_t)P;
    const float* lt = loo + row * (size_t)P1;
    double s1 = 0.0, s2 = 0.0;
    for (int q = lane; q < P1; q += 64) {
        int i, j;
        pftaxa::pair_of(q, N - 1, &i, &j);
        i += i >= t ? 1 : 0;
        j += j >= t ? 1 : 0;
        const double d = (double)lt[q] - (double)f[pftaxa::pair_index(i, j, N)];
        s1 += d;
        s2 += d * d;
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if (lane == 0) {
        influence[row] = (float)sqrt(s2 / (double)P1);
        shift[row] = (float)(s1 / (double)P1);
    }
}

// grid (ceil(P / LP_THREADS), nb), block LP_THREADS
__global__ __launch_bounds__(LP_THREADS) void k_loo_pair(const float* full, const float* loo, float* context, int N) {
    const int P = N * (N - 1) / 2, P1 = (N - 1) * (N - 2) / 2;
    const int p = blockIdx.x * LP_THREADS + threadIdx.x;
    if (p >= P) return;
    const size_t b = blockIdx.y;
    int i, j;
    pftaxa::pair_of(p, N, &i, &j);
    const double f = (double)full[b * (size_t)P + p];
    const float* lb = loo + b * (size_t)N * (size_t)P1;
    double s2 = 0.0;
    for (int t = 0; t < N; ++t) {
        if (t == i || t == j) continue;
        const double d = (double)lb[(size_t)t * P1 + (size_t)pftaxa::loo_pair_index(i, j, t, N)] - f;
        s2 += d * d;
    }
    context[b * (size_t)P + p] = (float)sqrt(s2 / (double)(N - 2));
}

// Asynchronous on `s`: full [B][P], loo [B][N][P1] -> influence [B][N], shift [B][N], context [B][P]; N >= 3.
inline hipError_t launch_loo_stats(hipStream_t s, const float* full, const float* loo, int B, int N, float* influence, float* shift,
                                   float* context) {
    const size_t rows = (size_t)B * N, P = (size_t)N * (N - 1) / 2, P1 = (size_t)(N - 1) * (N - 2) / 2;
    hipLaunchKernelGGL(k_loo_taxon, dim3((unsigned)((rows + LT_WAVES - 1) / LT_WAVES)), dim3(64 * LT_WAVES), 0, s, full, loo,
                       influence, shift, rows, N);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (int b0 = 0; b0 < B; b0 += GT_MAX_Y) {
        hipLaunchKernelGGL(k_loo_pair, dim3((unsigned)((P + LP_THREADS - 1) / LP_THREADS), (unsigned)std::min(GT_MAX_Y, B - b0)),
                           dim3(LP_THREADS), 0, s, full + (size_t)b0 * P, loo + (size_t)b0 * N * P1, context + (size_t)b0 * P, N);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pft
