// Query placement (pf_forward_place, pf_place_stats_device): the reductions of "add one in", the mirror of leave-one-out.
// An alignment of M rows is a backbone - its first N rows - and Q = M - N queries, its last rows.  Set q is the backbone
// with query q alone: the rows (0, .., N - 1, N + q), cut by k_gather_taxa (pf_taxa.hip.h) like any other row subset, so
// there is no gather here.  phyloformer_amd/place.py::place_stats is the host twin.
//
// whole float [B][P_M], base float [B][P_N], sets float [B][Q][P_{N+1}], P_n = n (n - 1) / 2, all in the reference's
// pair order (pf_taxa_host.h).  In set q the query is row N, so its distance to backbone row i is the LAST entry of
// row i, pair_{N+1}(i, N), and backbone pair (i, j) of index p among N rows has index p + i among N + 1 (every earlier
// row is one entry longer).  With delta_q(i, j) = sets[q][p + i] - base[p] (exact in double):
//
//   place[b][q][i]  = sets[b][q][pair_{N+1}(i, N)]                                   a copy: the bits of the set's
//   joint[b][q]     = sqrt( mean_i (whole[b][pair_M(i, N + q)] - place[b][q][i])^2 )  how far the OTHER queries' presence
//                                                                                    moves q's distances to the backbone
//   shift[b][q]     = mean over the P_N backbone pairs of delta_q                    signed
//   disturb[b][q]   = sqrt( mean over the P_N backbone pairs of delta_q^2 )          how far q moves the backbone's own
//
// Accumulated in double, rounded to float once, no atomics: the bits are a function of (N, Q, values) only.
//   k_place_rows      one wave per (b, q): lane l copies and adds the rows l, l + 64, ... in that order, the 64 lane
//                     sums meet in pft::wave_sum_f64's fixed xor tree.
//   k_place_backbone  one wave per (b, q): lane l adds the pairs l, l + 64, ... (coalesced along the set and the base).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_taxa.hip.h"

namespace pfpl {

constexpr int PL_WAVES = 4;            // (b, q) rows per workgroup

// grid ceil(rows / PL_WAVES), block 64 * PL_WAVES; rows = B * Q
__global__ __launch_bounds__(64 * PL_WAVES) void k_place_rows(const float* whole, const float* sets, float* place, float* joint,
                                                             size_t rows, int N, int Q) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * PL_WAVES + (threadIdx.x >> 6);      // b * Q + q
    if (row >= rows) return;                                                    // (wave-uniform)
    const size_t b = row / (size_t)Q;
    const int q = (int)(row - b * (size_t)Q);
    const int M = N + Q;
    const size_t PM = (size_t)M * (M - 1) / 2, P1 = (size_t)(N + 1) * N / 2;
    const float* w = whole + b * PM;
    const float* st = sets + row * P1;
    float* pl = place + row * (size_t)N;
    double s2 = 0.0;
    for (int i = lane; i < N; i += 64) {
        const float v = st[pftaxa::pair_index(i, N, N + 1)];
        pl[i] = v;
        const double d = (double)w[pftaxa::pair_index(i, N + q, M)] - (double)v;
        s2 += d * d;
    }
    s2 = pft::wave_sum_f64(s2);
    if (lane == 0) joint[row] = (float)sqrt(s2 / (double)N);
}

// grid ceil(rows / PL_WAVES), block 64 * PL_WAVES; rows = B * Q
__global__ __launch_bounds__(64 * PL_WAVES) void k_place_backbone(const float* base, const float* sets, float* disturb, float* shift,
                                                                 size_t rows, int N, int Q) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * PL_WAVES + (threadIdx.x >> 6);      // b * Q + q
    if (row >= rows) return;                                                    // (wave-uniform)
    const size_t b = row / (size_t)Q;
    const int PN = N * (N - 1) / 2;
    const size_t P1 = (size_t)(N + 1) * N / 2;
    const float* bs = base + b * (size_t)PN;
    const float* st = sets + row * P1;
    double s1 = 0.0, s2 = 0.0;
    for (int p = lane; p < PN; p += 64) {
        int i, j;
        pftaxa::pair_of(p, N, &i, &j);
        const double d = (double)st[p + i] - (double)bs[p];
        s1 += d;
        s2 += d * d;
    }
    s1 = pft::wave_sum_f64(s1);
    s2 = pft::wave_sum_f64(s2);
    if (lane == 0) {
        disturb[row] = (float)sqrt(s2 / (double)PN);
        shift[row] = (float)(s1 / (double)PN);
    }
}

// Asynchronous on `s`: whole [B][P_M], base [B][P_N], sets [B][Q][P_{N+1}] -> place [B][Q][N], disturb, shift,
// joint [B][Q]; N >= 2, Q >= 1.
inline hipError_t launch_place_stats(hipStream_t s, const float* whole, const float* base, const float* sets, int B, int N, int Q,
                                     float* place, float* disturb, float* shift, float* joint) {
    const size_t rows = (size_t)B * Q;
    const dim3 grid((unsigned)((rows + PL_WAVES - 1) / PL_WAVES)), block(64 * PL_WAVES);
    hipLaunchKernelGGL(k_place_rows, grid, block, 0, s, whole, sets, place, joint, rows, N, Q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_place_backbone, grid, block, 0, s, base, sets, disturb, shift, rows, N, Q);
    return hipGetLastError();
}

}  // namespace pfpl
