// BIONJ on the device (pf_bionj_joins, pf_bionj_joins_device): float preds [B][P_N] -> the join
// tables slots int32 / lengths double [B][2 (N - 3) + 3], bit for bit those of bionj.py::bionj_joins.  The bodies are
// pf_bionj_host.h's, shared with the CPU, as is the list of the state's arrays; this file is the launches.  No atomics,
// no cooperative launch, no copy to the host and no synchronisation between joins: the host knows m = N - t for every
// join t and enqueues the whole sequence.
//   k_bionj_init    grid (<= INIT_GROUPS, sources): d and v [N][N] from preds, the first list of active rows, the
//                   labels, the flag of a source with a NaN or an infinity (every later kernel returns at once for it)
// per join t, m = N - t active positions:
//   k_nj_rowsum     pf_nj.hip.h's, on the same d, r and list
//   k_bionj_qmin    grid (min(m, Q_GROUPS), sources): every thread the minimum key (q, x, y) of its pairs y < x, then
//                   the workgroup's in LDS, one partial minimum per workgroup
//   k_bionj_pick    the same grid and the same pairs per thread: every workgroup reduces the partial minima to q*,
//                   evaluates q again and keeps the first pair of the scan with q <= q* + EPS, one per workgroup
//   k_bionj_join    grid (1, sources): the first of those pairs, the join's record with lambda (one thread, broadcast
//                   through LDS), then row and column rx of d and v and the next list of active rows by all threads
//   k_bionj_final   one thread per source: the trifurcation
// Both minima are taken on total orders, so the LDS tree gives the same key as any other order would.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_bionj_host.h"
#include "pf_nj.hip.h"

namespace pfbionj {

using pfnj::INIT_GROUPS;
using pfnj::INIT_THREADS;
using pfnj::JOIN_THREADS;
using pfnj::Q_GROUPS;
using pfnj::Q_THREADS;
using pfnj::ROW_THREADS;
constexpr int BIONJ_MAX_Y = pfnj::NJ_MAX_Y;        // sources per launch (grid y)

__global__ __launch_bounds__(INIT_THREADS) void k_bionj_init(Args a) {
    init_elems(a, (size_t)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, INIT_THREADS);
}

__global__ __launch_bounds__(Q_THREADS) void k_bionj_qmin(Args a, int m, int t) {
    __shared__ Key keys[Q_THREADS];
    keys[threadIdx.x] = qmin_thread(a, m, t, (size_t)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, Q_THREADS);
    pfnj::reduce_keys<Q_THREADS>(keys);
    if (threadIdx.x == 0) a.nj.part[(size_t)blockIdx.y * (size_t)a.nj.part_cap + blockIdx.x] = keys[0];
}

__global__ __launch_bounds__(Q_THREADS) void k_bionj_pick(Args a, int m, int t) {
    __shared__ Key keys[Q_THREADS];
    const size_t src = (size_t)blockIdx.y;
    keys[threadIdx.x] = part_thread_key(a, a.nj.part, src, (int)gridDim.x, (int)threadIdx.x, Q_THREADS);
    pfnj::reduce_keys<Q_THREADS>(keys);
    const double qstar = keys[0].v;
    __syncthreads();                                         // everyone has read keys[0] before it is written again
    keys[threadIdx.x] = pick_thread(a, m, t, src, qstar, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, Q_THREADS);
    pfnj::reduce_keys<Q_THREADS>(keys);
    if (threadIdx.x == 0) a.part_at[src * (size_t)a.nj.part_cap + blockIdx.x] = keys[0];
}

__global__ __launch_bounds__(JOIN_THREADS) void k_bionj_join(Args a, int m, int t, int G) {
    __shared__ Key keys[JOIN_THREADS];
    __shared__ Join join;
    const size_t src = (size_t)blockIdx.y;
    keys[threadIdx.x] = part_thread_key(a, a.part_at, src, G, (int)threadIdx.x, JOIN_THREADS);
    pfnj::reduce_keys<JOIN_THREADS>(keys);
    if (threadIdx.x == 0) join = join_record(a, m, t, src, keys[0]);
    __syncthreads();
    const Join j = join;
    join_update(a, m, t, src, j, (int)threadIdx.x, JOIN_THREADS);
}

__global__ __launch_bounds__(64) void k_bionj_final(Args a, int B) {
    const int src = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (src < B) final_record(a, (size_t)src);
}

// Asynchronous on `s`: the whole join sequence of B <= BIONJ_MAX_Y sources of N >= 3 sequences.
inline hipError_t launch_bionj(hipStream_t s, const Args& a, int B) {
    const int N = a.nj.N;
    hipError_t e = hipMemsetAsync(a.nj.flag, 0, (size_t)B, s);
    if (e != hipSuccess) return e;
    const int64_t NN = (int64_t)N * N;
    const unsigned gi = (unsigned)std::min<int64_t>(INIT_GROUPS, (NN + INIT_THREADS - 1) / INIT_THREADS);
    hipLaunchKernelGGL(k_bionj_init, dim3(gi, (unsigned)B), dim3(INIT_THREADS), 0, s, a);
    for (int t = 0; t < N - 3; ++t) {
        const int m = N - t, G = std::min(m, Q_GROUPS);
        hipLaunchKernelGGL(pfnj::k_nj_rowsum, dim3((unsigned)((m + ROW_THREADS - 1) / ROW_THREADS), (unsigned)B), dim3(ROW_THREADS), 0, s, a.nj, m, t);
        hipLaunchKernelGGL(k_bionj_qmin, dim3((unsigned)G, (unsigned)B), dim3(Q_THREADS), 0, s, a, m, t);
        hipLaunchKernelGGL(k_bionj_pick, dim3((unsigned)G, (unsigned)B), dim3(Q_THREADS), 0, s, a, m, t);
        hipLaunchKernelGGL(k_bionj_join, dim3(1, (unsigned)B), dim3(JOIN_THREADS), 0, s, a, m, t, G);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_bionj_final, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, a, B);
    return hipGetLastError();
}

}  // namespace pfbionj
