// Delta scores on the device (pf_delta, pf_delta_device): float preds [B][P_N] -> pair_sum int64
// [B][P_N], hist int64 [B][K], nonfinite uint8 [B], bit for bit those of pf_delta_host.h::run_serial and of
// delta.py::delta_py.  The quartet's arithmetic is pf_delta_host.h's; this file is the kernels and their launches.
//   k_delta_flag      grid (sources): the flag of a source with a NaN or an infinity
//   k_delta_quartets  the product's kernel: one workgroup per (source, pair a < b), every quartet evaluated once, its q
//                     added to its six pairs through registers, LDS atomics and one global atomic (see at the kernel)
//   k_delta_pairs     option "delta_atomic" = 0, the design without atomics on pair_sum that the product's was measured
//                     against: one workgroup per (source, pair i < j), the owner of pair_sum[i, j]: rows i and j of the
//                     matrix in LDS, the threads stride over the pairs u < v of all sequences - consecutive threads read
//                     consecutive distances d_uv - and skip those that touch i or j; q is summed in registers, then
//                     over the workgroup, and stored once; a quartet is evaluated by its six owners.  The histogram
//                     counts a quartet at one of them, j < u.
// Both count the histogram in LDS and add a workgroup's non-empty bins to the source's by 64-bit atomics; every sum is
// of integers, so no order shows and the two kernels give the same arrays.  A flagged source's arrays are zeros.
// A call's (source, pair) items are cut into launches of at most LAUNCH_EVALS partner pairs, all on one stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_delta_host.h"

namespace pfdelta {

constexpr int THREADS = 256;
// The partner pairs of one launch, C(N - 2, 2) counted for every item: k_delta_pairs evaluates them all, at 5.6e11 a
// second from 512 sequences on; k_delta_quartets evaluates C(N - b - 1, 2) of them, a third over a row of items, at
// 1.62e11 a second (profiles/delta_bench.txt).  2^35 bounds a launch by 0.21 s; at 2,048 sequences the longest, the
// first, takes about 0.07 s.
constexpr int64_t LAUNCH_EVALS = (int64_t)1 << 35;

struct Args {
    const float* preds;     // [B][P]
    int64_t* pair_sum;      // [B][P]
    int64_t* hist;          // [B][K], zeroed before the first launch
    uint8_t* flag;          // [B]
    int64_t P, items;       // pairs of a source, B * P
    int N, K;
};

__global__ __launch_bounds__(THREADS) void k_delta_flag(Args a) {
    const float* pr = a.preds + (size_t)blockIdx.x * (size_t)a.P;
    int bad = 0;
    for (int64_t e = threadIdx.x; e < a.P; e += THREADS) bad |= nonfinite(pr[e]) ? 1 : 0;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) a.flag[blockIdx.x] = bad ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void k_delta_pairs(Args a, int64_t item0) {
    extern __shared__ __align__(8) float rows[];       // d(i, x), then d(j, x), x in [0, N)
    __shared__ unsigned int bins[MAX_K];
    __shared__ int64_t part[THREADS / 64];
    const int64_t item = item0 + (int64_t)blockIdx.x;
    if (item >= a.items) return;
    const int64_t src = item / a.P, p = item - src * a.P;
    const int tid = (int)threadIdx.x, N = a.N;
    if (a.flag[src]) {
        if (tid == 0) a.pair_sum[item] = 0;
        return;
    }
    int i, j;
    pair_of(p, N, &i, &j);
    const float* pr = a.preds + (size_t)src * (size_t)a.P;
    float* ri = rows;
    float* rj = rows + N;
    for (int x = tid; x < N; x += THREADS) {
        ri[x] = x == i ? 0.0f : pr[x < i ? row_start(x, N) + (i - x - 1) : row_start(i, N) + (x - i - 1)];
        rj[x] = x == j ? 0.0f : pr[x < j ? row_start(x, N) + (j - x - 1) : row_start(j, N) + (x - j - 1)];
    }
    if (tid < MAX_K) bins[tid] = 0;
    __syncthreads();
    const double dij = (double)rj[i];
    int64_t sum = 0;
    int u = 0, v = 1 + tid;
    for (int64_t e = tid; e < a.P; e += THREADS, v += THREADS) {
        while (v >= N) { v -= N; ++u; v += u + 1; }                   // (e < P: the row exists)
        if (u == i || u == j || v == i || v == j) continue;
        const int64_t q = quartet_q(dij + (double)pr[e], (double)ri[u] + (double)rj[v], (double)ri[v] + (double)rj[u]);
        sum += q;
        if (u > j) atomicAdd(&bins[bin_of(q, a.K)], 1u);
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t s = 0;
        for (int w = 0; w < THREADS / 64; ++w) s += part[w];
        a.pair_sum[item] = s;
    }
    if (tid < a.K && bins[tid])
        atomicAdd(reinterpret_cast<unsigned long long*>(a.hist + src * a.K + tid), (unsigned long long)bins[tid]);
}

// The design with atomics, 1.2 times as fast as k_delta_pairs at 200 sequences, 1.6 times at 1,024 and 1.8 times at
// 2,048 (tools/delta_bench.py).  One workgroup per (source, pair a < b): the threads stride over the pairs c < d behind
// b, so a quartet is evaluated once.  Its q goes to the pair (a, b) through registers, to (a, c) and (b, c) through a
// register that is added to LDS when the thread's c changes, to (a, d) and (b, d) by 64-bit LDS atomics, to (c, d) by a
// 64-bit global atomic (consecutive threads, consecutive addresses); the workgroup then adds its LDS sums to pair_sum,
// zeroed before the first launch.
__global__ __launch_bounds__(THREADS) void k_delta_quartets(Args a, int64_t item0) {
    extern __shared__ __align__(8) float rows[];       // d(a, x), d(b, x), then the sums of (a, x) and (b, x), x in [0, N)
    __shared__ unsigned int bins[MAX_K];
    __shared__ int64_t part[THREADS / 64];
    const int64_t item = item0 + (int64_t)blockIdx.x;
    if (item >= a.items) return;
    const int64_t src = item / a.P, p = item - src * a.P;
    const int tid = (int)threadIdx.x, N = a.N;
    if (a.flag[src]) return;
    int i, j;
    pair_of(p, N, &i, &j);
    if (j >= N - 2) return;                            // no pair behind b
    const float* pr = a.preds + (size_t)src * (size_t)a.P;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(a.pair_sum + src * a.P);
    float* ri = rows;
    float* rj = rows + N;
    unsigned long long* acc_i = reinterpret_cast<unsigned long long*>(rows + 2 * (size_t)N);
    unsigned long long* acc_j = acc_i + N;
    for (int x = tid; x < N; x += THREADS) {
        ri[x] = x <= i ? 0.0f : pr[row_start(i, N) + (x - i - 1)];
        rj[x] = x <= j ? 0.0f : pr[row_start(j, N) + (x - j - 1)];
        acc_i[x] = 0; acc_j[x] = 0;
    }
    if (tid < MAX_K) bins[tid] = 0;
    __syncthreads();
    const double dij = (double)ri[j];
    int64_t sum = 0, run = 0;
    int u = j + 1, v = j + 2 + tid, run_u = -1;
    for (int64_t e = row_start(j + 1, N) + tid; e < a.P; e += THREADS, v += THREADS) {
        while (v >= N) { v -= N; ++u; v += u + 1; }
        if (u != run_u) {
            if (run) { atomicAdd(&acc_i[run_u], (unsigned long long)run); atomicAdd(&acc_j[run_u], (unsigned long long)run); }
            run = 0; run_u = u;
        }
        const int64_t q = quartet_q(dij + (double)pr[e], (double)ri[u] + (double)rj[v], (double)ri[v] + (double)rj[u]);
        if (q) {
            sum += q; run += q;
            atomicAdd(&acc_i[v], (unsigned long long)q);
            atomicAdd(&acc_j[v], (unsigned long long)q);
            atomicAdd(&out[e], (unsigned long long)q);
        }
        atomicAdd(&bins[bin_of(q, a.K)], 1u);
    }
    if (run) { atomicAdd(&acc_i[run_u], (unsigned long long)run); atomicAdd(&acc_j[run_u], (unsigned long long)run); }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t s = 0;
        for (int w = 0; w < THREADS / 64; ++w) s += part[w];
        if (s) atomicAdd(&out[p], (unsigned long long)s);
    }
    for (int x = j + 1 + tid; x < N; x += THREADS) {
        if (acc_i[x]) atomicAdd(&out[row_start(i, N) + (x - i - 1)], acc_i[x]);
        if (acc_j[x]) atomicAdd(&out[row_start(j, N) + (x - j - 1)], acc_j[x]);
    }
    if (tid < a.K && bins[tid])
        atomicAdd(reinterpret_cast<unsigned long long*>(a.hist + src * a.K + tid), (unsigned long long)bins[tid]);
}

// Asynchronous on `s`: B sources of N sequences, K bins (refused(B, N, K) == 0); `atomic`: by k_delta_quartets.
inline hipError_t launch_delta(hipStream_t s, const float* preds, int B, int N, int K, int64_t* pair_sum, int64_t* hist, uint8_t* flag,
                               bool atomic = true) {
    Args a{};
    a.preds = preds; a.pair_sum = pair_sum; a.hist = hist; a.flag = flag;
    a.N = N; a.K = K;
    a.P = (int64_t)N * (N - 1) / 2;
    a.items = (int64_t)B * a.P;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * (size_t)K * sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_delta_flag, dim3((unsigned)B), dim3(THREADS), 0, s, a);
    const int64_t evals = (int64_t)(N - 2) * (N - 3) / 2;             // of one item
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(LAUNCH_EVALS / evals, (int64_t)1 << 30));
    if (atomic && (e = hipMemsetAsync(pair_sum, 0, (size_t)a.items * sizeof(int64_t), s)) != hipSuccess) return e;
    const size_t lds = 2 * (size_t)N * sizeof(float) + (atomic ? 2 * (size_t)N * sizeof(int64_t) : 0);
    for (int64_t item0 = 0; item0 < a.items; item0 += per) {
        const dim3 grid((unsigned)std::min(per, a.items - item0));
        hipLaunchKernelGGL(atomic ? k_delta_quartets : k_delta_pairs, grid, dim3(THREADS), lds, s, a, item0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace pfdelta
