// Neighbour joining on the device (pf_nj_joins, pf_nj_joins_device): float preds [B][P_N] ->
// the join tables slots int32 / lengths double [B][2 (N - 3) + 3], bit for bit those of nj.py::nj_joins.  The bodies are
// pf_nj_host.h's, shared with the CPU, as is the list of the state's arrays; this file is the launches.  No atomics, no cooperative launch, no copy to the
// host and no synchronisation between joins: the host knows m = N - t for every join t and enqueues the whole sequence.
//   k_nj_init     grid (<= INIT_GROUPS, sources): d [N][N] from preds, the first list of active slots, the flag of a
//                 source with a NaN or an infinity (every later kernel returns at once for a flagged source)
// per join t, m = N - t active slots:
//   k_nj_rowsum   grid (ceil(m / ROW_THREADS), sources), one thread per row: numpy's pairwise sum of the row, whole, by
//                 one thread; neighbouring lanes read neighbouring addresses (the symmetric element)
//   k_nj_qmin     grid (min(m, Q_GROUPS), sources): every thread the minimum key (q, a, b) of its elements of Q, then the
//                 workgroup's in LDS, one partial minimum per workgroup
//   k_nj_join     grid (1, sources): the minimum of the partial minima, the join's record (one thread, broadcast
//                 through LDS), then row and column ia of d and the next list of active slots by all threads
//   k_nj_final    one thread per source: the trifurcation
// The minimum is taken on a total order, so the LDS tree (the step the CPU test runs too) gives the same key as any
// other order would.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_nj_host.h"

namespace pfnj {

constexpr int INIT_THREADS = 256, INIT_GROUPS = 1024;
constexpr int ROW_THREADS = 64;
constexpr int Q_THREADS = 256;
constexpr int JOIN_THREADS = 256;
constexpr int NJ_MAX_Y = 65535;        // sources per launch (grid y)

__global__ __launch_bounds__(INIT_THREADS) void k_nj_init(Args a) {
    init_elems(a, (size_t)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, INIT_THREADS);
}

__global__ __launch_bounds__(ROW_THREADS) void k_nj_rowsum(Args a, int m, int t) {
    const int row = (int)blockIdx.x * ROW_THREADS + (int)threadIdx.x;
    if (row < m) row_sum(a, m, t, (size_t)blockIdx.y, row);
}

// the workgroup's minimum of keys[0 .. THREADS) into keys[0] (every kernel that takes a minimum, pf_bme.hip.h's too)
template <int THREADS>
__device__ inline void reduce_keys(Key* keys) {
    for (int s = reduce_first_step(THREADS); s > 0; s >>= 1) {
        __syncthreads();
        reduce_step(keys, (int)threadIdx.x, s, THREADS);
    }
    __syncthreads();
}

__global__ __launch_bounds__(Q_THREADS) void k_nj_qmin(Args a, int m, int t) {
    __shared__ Key keys[Q_THREADS];
    keys[threadIdx.x] = qmin_thread(a, m, t, (size_t)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, Q_THREADS);
    reduce_keys<Q_THREADS>(keys);
    if (threadIdx.x == 0) a.part[(size_t)blockIdx.y * (size_t)a.part_cap + blockIdx.x] = keys[0];
}

__global__ __launch_bounds__(JOIN_THREADS) void k_nj_join(Args a, int m, int t, int G) {
    __shared__ Key keys[JOIN_THREADS];
    __shared__ Join join;
    const size_t src = (size_t)blockIdx.y;
    keys[threadIdx.x] = join_thread_key(a, src, G, (int)threadIdx.x, JOIN_THREADS);
    reduce_keys<JOIN_THREADS>(keys);
    if (threadIdx.x == 0) join = join_record(a, m, t, src, keys[0]);
    __syncthreads();
    const Join j = join;
    join_update(a, m, t, src, j, (int)threadIdx.x, JOIN_THREADS);
}

__global__ __launch_bounds__(64) void k_nj_final(Args a, int B) {
    const int src = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (src < B) final_record(a, (size_t)src);
}

// Asynchronous on `s`: the whole join sequence of B <= NJ_MAX_Y sources of N >= 3 sequences.
inline hipError_t launch_nj(hipStream_t s, const Args& a, int B) {
    const int N = a.N;
    hipError_t e = hipMemsetAsync(a.flag, 0, (size_t)B, s);
    if (e != hipSuccess) return e;
    const int64_t NN = (int64_t)N * N;
    const unsigned gi = (unsigned)std::min<int64_t>(INIT_GROUPS, (NN + INIT_THREADS - 1) / INIT_THREADS);
    hipLaunchKernelGGL(k_nj_init, dim3(gi, (unsigned)B), dim3(INIT_THREADS), 0, s, a);
    for (int t = 0; t < N - 3; ++t) {
        const int m = N - t, G = std::min(m, Q_GROUPS);
        hipLaunchKernelGGL(k_nj_rowsum, dim3((unsigned)((m + ROW_THREADS - 1) / ROW_THREADS), (unsigned)B), dim3(ROW_THREADS), 0, s, a, m, t);
        hipLaunchKernelGGL(k_nj_qmin, dim3((unsigned)G, (unsigned)B), dim3(Q_THREADS), 0, s, a, m, t);
        hipLaunchKernelGGL(k_nj_join, dim3(1, (unsigned)B), dim3(JOIN_THREADS), 0, s, a, m, t, G);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_nj_final, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, a, B);
    return hipGetLastError();
}

}  // namespace pfnj
