// Reductions of a site map (pf_forward_site_profile, pf_site_moments_device): from the terms of the site mean,
//
//   map float [nb][P][L],   map[b][p][l] = softplus(head logit of pair p at site l)      (distance[p] = mean_l map[p][l])
//
// to the spread of every distance's site mean and to every site's share of the distances:
//
//   se      float [nb][P]   se[p] = sqrt( sum_l (map[p][l] - m[p])^2 / (L (L - 1)) ),  m[p] = mean_l map[p][l];  L = 1: 0
//   profile float [nb][L]   profile[l] = mean_p map[p][l]
//
// (phyloformer_amd/siteprofile.py::site_moments is the host twin).  Everything is accumulated in double and rounded to
// float once.  No floating-point atomics: as for every other reduction of this library the result bits are a function
// of (P, L) and the values only, never of the batch position, the chunking or the grid.
//
//   k_site_se        one wave per row (b, p), coalesced along l.  Two passes over the row (the second one hits L2 / L1):
//                    lane j sums sites j, j + 64, ... in that order, the 64 lane sums meet in a fixed xor tree.
//   k_site_colpart   the P rows are cut into segments of seg_rows(P) rows - a function of P alone; a workgroup of one wave
//                    owns (alignment, segment, 64 consecutive sites) and adds the segment's rows in row order:
//                    part double [nb][nseg][L].  A lone 20 x 200 alignment (190 x 200) spreads over 24 segments x 4 site
//                    tiles, a lone 200 x 500 one (19,900 x 500) over 256 x 8.
//   k_site_colfin    adds the segments in index order, divides by P.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace pfm {

constexpr int SM_WAVES = 4;            // rows per workgroup of k_site_se
constexpr int SM_TILE = 64;            // sites per workgroup of k_site_colpart (one wave: 256 contiguous bytes per row)
constexpr int SM_MIN_SEG = 8;          // rows per segment of a small P
constexpr int SM_MAX_SEGS = 256;       // segments of a large P

// rows per profile segment and their number: functions of P alone
inline int seg_rows(int P) { return std::max(SM_MIN_SEG, (P + SM_MAX_SEGS - 1) / SM_MAX_SEGS); }
inline int seg_count(int P) { return (P + seg_rows(P) - 1) / seg_rows(P); }
// doubles of k_site_colpart's partial sums for nb alignments
inline size_t part_count(int nb, int P, int L) { return (size_t)nb * (size_t)seg_count(P) * (size_t)L; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// grid ceil(rows / SM_WAVES), block 64 * SM_WAVES
__global__ __launch_bounds__(64 * SM_WAVES) void k_site_se(const float* map, float* se, size_t rows, int L) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * SM_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;                                           // (wave-uniform)
    const float* m = map + row * (size_t)L;
    double s = 0.0;
    for (int l = lane; l < L; l += 64) s += (double)m[l];
    const double mean = wave_sum_f64(s) / (double)L;
    double q = 0.0;
    for (int l = lane; l < L; l += 64) {
        const double d = (double)m[l] - mean;
        q += d * d;
    }
    q = wave_sum_f64(q);
    if (lane == 0) se[row] = L > 1 ? (float)sqrt(q / ((double)L * (double)(L - 1))) : 0.f;
}

// grid (ceil(L / SM_TILE), nseg, nb), block SM_TILE
__global__ __launch_bounds__(SM_TILE) void k_site_colpart(const float* map, double* part, int P, int L, int seg, int nseg) {
    const int l = blockIdx.x * SM_TILE + threadIdx.x;
    if (l >= L) return;
    const int sg = blockIdx.y, b = blockIdx.z;
    const int p0 = sg * seg, p1 = min(P, p0 + seg);
    const float* m = map + ((size_t)b * P + p0) * (size_t)L + l;
    double s = 0.0;
#pragma unroll 4
    for (int p = p0; p < p1; ++p, m += L) s += (double)*m;
    part[((size_t)b * nseg + sg) * (size_t)L + l] = s;
}

// grid (ceil(L / 256), nb), block 256
__global__ __launch_bounds__(256) void k_site_colfin(const double* part, float* profile, int P, int L, int nseg) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int b = blockIdx.y;
    const double* q = part + (size_t)b * nseg * (size_t)L + l;
    double s = 0.0;
    for (int sg = 0; sg < nseg; ++sg) s += q[(size_t)sg * L];
    profile[(size_t)b * L + l] = (float)(s / (double)P);
}

// Asynchronous on `s`: map [nb][P][L] -> se [nb][P], profile [nb][L]; part holds part_count(nb, P, L) doubles.
// nb <= 65535 (grid y / z): the caller cuts larger batches.
inline hipError_t launch_site_moments(hipStream_t s, const float* map, int nb, int P, int L, double* part, float* se,
                                      float* profile) {
    const size_t rows = (size_t)nb * P;
    const int seg = seg_rows(P), nseg = seg_count(P);
    hipLaunchKernelGGL(k_site_se, dim3((unsigned)((rows + SM_WAVES - 1) / SM_WAVES)), dim3(64 * SM_WAVES), 0, s, map, se, rows, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_site_colpart, dim3((unsigned)((L + SM_TILE - 1) / SM_TILE), (unsigned)nseg, (unsigned)nb), dim3(SM_TILE),
                       0, s, map, part, P, L, seg, nseg);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_site_colfin, dim3((unsigned)((L + 255) / 256), (unsigned)nb), dim3(256), 0, s, part, profile, P, L, nseg);
    return hipGetLastError();
}

}  // namespace pfm
