// Balanced minimum-evolution NNI refinement on the device (pf_bme_nni, pf_bme_nni_device): float
// preds [B][P_N] and start tables -> refined join tables with balanced branch lengths, bit for bit those of the serial
// run of the same bodies (pf_bme_nni_host) and, from the final from-scratch table, of bme.py.  The bodies and the case
// analysis of the update are pf_bme_host.h's, shared with the CPU, and so are the lists of the state's arrays with the
// bytes and the device spans they give; this file is the launches.  No atomics, no cooperative launch; the host looks
// at the flags once per round of ROUND_STEPS steps.
//   k_bme_init     grid (<= INIT_GROUPS, sources): d [N][N] from preds, the status of a source with a NaN or an infinity
//   k_bme_build    grid (ceil(N / 256), rows, sources): M[X][j] from depth and d for the sources marked `rebuild`; lane j
//                  reads d[i][j], neighbouring lanes neighbouring addresses
// per step:
//   k_bme_eval     grid (ceil(edges / EVAL_EDGES), sources): 6 threads per edge form its q (one pairwise sum each), then
//                  2 per internal edge its keys (delta, c, k), then the workgroup's minimum in LDS
//   k_bme_move     grid (1, sources): the minimum of the partial minima, the decision and the swap (one thread,
//                  broadcast through LDS), then the case and h of every row by all threads
//   k_bme_update   grid (ceil(nodes / 256), rows, sources): one thread per (row, node): depth, and M for a leaf
// at the end:
//   k_bme_lengths  grid (ceil(edges / 256), sources): the balanced length of every edge from q
// Every kernel returns at once for a done or flagged source.  The minimum is taken on a total order, so the LDS tree
// (the step the CPU test runs too) gives the same key as any other order would.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_bme_host.h"
#include "pf_nj.hip.h"

namespace pfbme {

constexpr int INIT_GROUPS = 1024;          // (THREADS, EVAL_EDGES, SPR_EVAL_EDGES: pf_bme_host.h, the state's sizes hang on them)
constexpr int BME_MAX_Z = 65535;           // sources per launch (grid y or z)

__global__ __launch_bounds__(THREADS) void k_bme_init(Args a) {
    init_elems(a, (size_t)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, THREADS);
}

__global__ __launch_bounds__(THREADS) void k_bme_build(Args a) {
    const int j = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (j < a.N) build_elem(a, (size_t)blockIdx.z, (int64_t)blockIdx.y, j);
}

__global__ __launch_bounds__(THREADS) void k_bme_eval(Args a) {
    __shared__ double lq[EVAL_EDGES * 6];
    __shared__ Key keys[THREADS];
    const size_t src = (size_t)blockIdx.y;
    eval_q_thread(a, src, (int)blockIdx.x, EVAL_EDGES, (int)threadIdx.x, THREADS, lq);
    __syncthreads();
    keys[threadIdx.x] = eval_key_thread(a, src, (int)blockIdx.x, EVAL_EDGES, (int)threadIdx.x, THREADS, lq);
    pfnj::reduce_keys<THREADS>(keys);
    if (threadIdx.x == 0) a.part[src * (size_t)a.part_cap + blockIdx.x] = keys[0];
}

__global__ __launch_bounds__(THREADS) void k_bme_move(Args a, int G) {
    __shared__ Key keys[THREADS];
    __shared__ Move move;
    const size_t src = (size_t)blockIdx.y;
    keys[threadIdx.x] = move_thread_key(a, src, G, (int)threadIdx.x, THREADS);
    pfnj::reduce_keys<THREADS>(keys);
    if (threadIdx.x == 0) move = move_decide(a, src, keys[0]);
    __syncthreads();
    const Move m = move;
    move_rowcase(a, src, m, (int)threadIdx.x, THREADS);
}

__global__ __launch_bounds__(THREADS) void k_bme_update(Args a) {
    const int v = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (v < (int)nodes_of(a.N)) update_elem(a, (size_t)blockIdx.z, (int64_t)blockIdx.y, v);
}

__global__ __launch_bounds__(THREADS) void k_bme_lengths(Args a) {
    const int e = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (e < (int)root_of(a.N)) edge_length(a, (size_t)blockIdx.y, e);
}

// asynchronous on `s`: d of B <= BME_MAX_Z sources (status zeroed by the caller)
inline hipError_t launch_init(hipStream_t s, const Args& a, int B) {
    const int64_t NN = (int64_t)a.N * a.N;
    const unsigned gi = (unsigned)std::min<int64_t>(INIT_GROUPS, (NN + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(k_bme_init, dim3(gi, (unsigned)B), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

// asynchronous on `s`: M from scratch for the marked sources, then one round of steps
inline hipError_t launch_round(hipStream_t s, const Args& a, int B) {
    const int N = a.N, G = a.part_cap;
    const unsigned rows = (unsigned)rows_of(N), nodes = (unsigned)nodes_of(N);
    hipLaunchKernelGGL(k_bme_build, dim3((unsigned)((N + THREADS - 1) / THREADS), rows, (unsigned)B), dim3(THREADS), 0, s, a);
    for (int step = 0; step < ROUND_STEPS; ++step) {
        hipLaunchKernelGGL(k_bme_eval, dim3((unsigned)G, (unsigned)B), dim3(THREADS), 0, s, a);
        hipLaunchKernelGGL(k_bme_move, dim3(1, (unsigned)B), dim3(THREADS), 0, s, a, G);
        hipLaunchKernelGGL(k_bme_update, dim3((nodes + THREADS - 1) / THREADS, rows, (unsigned)B), dim3(THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

inline hipError_t launch_lengths(hipStream_t s, const Args& a, int B) {
    hipLaunchKernelGGL(k_bme_lengths, dim3((unsigned)((root_of(a.N) + THREADS - 1) / THREADS), (unsigned)B), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

// ---- balanced subtree pruning and regrafting (pf_bme_spr, pf_bme_spr_device; the bodies and the
// order of a step are pf_bme_host.h's).  Per step, after k_bme_init once:
//   k_bme_number        grid (1, sources), one thread: the numbering of the rooted tree
//   k_bme_depth         grid (ceil(nodes / 256), rows, sources): one thread per (row, node)
//   k_bme_build         as above: M of every row (a finished source has cleared its `rebuild`)
//   k_bme_pairs         grid (ceil(rows / 16), ceil(rows / 16), sources): T by 16 x 16 tiles, M and the weights staged
//                       leaf by leaf of the pairwise sum through LDS (2 x 16 x 129 doubles = 33,024 bytes); a tile whose
//                       entries all share a leaf writes its zeros and leaves
//   k_bme_pairs_simple  grid (ceil(rows / 256), rows, sources): T, one thread per entry from global memory (the baseline;
//                       option "spr_pairs_simple")
//   k_bme_spr_eval      grid (ceil(edges / SPR_EVAL_EDGES), rows, sources): one thread per (S row, target edge), the
//                       workgroup's minimum key in LDS
//   k_bme_spr_move      grid (1, sources): the minimum of the partial minima; one thread decides and moves
// at the end k_bme_eval and k_bme_lengths as above, on depth and M of the final topology.

__global__ __launch_bounds__(64) void k_bme_number(SprArgs s) {
    if (threadIdx.x == 0) number_tree(s, (size_t)blockIdx.y);
}

__global__ __launch_bounds__(THREADS) void k_bme_depth(SprArgs s) {
    const int v = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (v < (int)nodes_of(s.b.N)) depth_elem(s, (size_t)blockIdx.z, (int64_t)blockIdx.y, v);
}

__global__ __launch_bounds__(PAIR_TILE * PAIR_TILE) void k_bme_pairs(SprArgs s) {
    __shared__ double lm[PAIR_TILE * PAIR_STRIDE], lw[PAIR_TILE * PAIR_STRIDE];
    const size_t src = (size_t)blockIdx.z;
    const int tx = (int)blockIdx.y, ty = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (spr_idle(s, src)) return;
    PairThread t;
    pairs_tile_begin(s, src, tx, ty, tid, t);
    if (__syncthreads_or(t.active)) {
        SumWalk walk;
        walk.start(s.b.N);
        int lo = 0, cnt = 0;
        for (int ev = walk.next(&lo, &cnt); ev; ev = walk.next(&lo, &cnt)) {
            if (ev == 2) { pairs_tile_add(t); continue; }
            __syncthreads();                                         // the leaf before has been read
            pairs_tile_stage(s, src, tx, ty, lo, cnt, tid, PAIR_TILE * PAIR_TILE, lm, lw);
            __syncthreads();
            pairs_tile_leaf(cnt, tid, lm, lw, t);
        }
    }
    pairs_tile_end(s, src, tx, ty, tid, t);
}

__global__ __launch_bounds__(THREADS) void k_bme_pairs_simple(SprArgs s) {
    const int64_t Y = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (Y < rows_of(s.b.N)) pairs_elem(s, (size_t)blockIdx.z, (int64_t)blockIdx.y, Y);
}

__global__ __launch_bounds__(THREADS) void k_bme_spr_eval(SprArgs s) {
    __shared__ Key keys[THREADS];
    const size_t src = (size_t)blockIdx.z;
    keys[threadIdx.x] = spr_eval_thread(s, src, (int64_t)blockIdx.y, (int)blockIdx.x, (int)threadIdx.x, THREADS);
    pfnj::reduce_keys<THREADS>(keys);
    if (threadIdx.x == 0) s.spart[src * (size_t)s.spart_cap + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = keys[0];
}

__global__ __launch_bounds__(THREADS) void k_bme_spr_move(SprArgs s) {
    __shared__ Key keys[THREADS];
    const size_t src = (size_t)blockIdx.y;
    keys[threadIdx.x] = spr_move_thread_key(s, src, (int)threadIdx.x, THREADS);
    pfnj::reduce_keys<THREADS>(keys);
    if (threadIdx.x == 0) spr_decide(s, src, keys[0]);
}

// asynchronous on `st`: one round of steps; `ev`, when not NULL, two events recorded around the pair table of the first
inline hipError_t launch_spr_round(hipStream_t st, const SprArgs& s, int B, bool pairs_simple, hipEvent_t* ev = nullptr) {
    const int N = s.b.N;
    const unsigned rows = (unsigned)rows_of(N), nodes = (unsigned)nodes_of(N), b = (unsigned)B;
    const unsigned tiles = (rows + PAIR_TILE - 1) / PAIR_TILE;
    for (int step = 0; step < ROUND_STEPS; ++step) {
        hipLaunchKernelGGL(k_bme_number, dim3(1, b), dim3(64), 0, st, s);
        hipLaunchKernelGGL(k_bme_depth, dim3((nodes + THREADS - 1) / THREADS, rows, b), dim3(THREADS), 0, st, s);
        hipLaunchKernelGGL(k_bme_build, dim3((unsigned)((N + THREADS - 1) / THREADS), rows, b), dim3(THREADS), 0, st, s.b);
        if (ev && step == 0) hipEventRecord(ev[0], st);
        if (pairs_simple) hipLaunchKernelGGL(k_bme_pairs_simple, dim3((rows + THREADS - 1) / THREADS, rows, b), dim3(THREADS), 0, st, s);
        else hipLaunchKernelGGL(k_bme_pairs, dim3(tiles, tiles, b), dim3(PAIR_TILE * PAIR_TILE), 0, st, s);
        if (ev && step == 0) hipEventRecord(ev[1], st);
        hipLaunchKernelGGL(k_bme_spr_eval, dim3((unsigned)eval_groups(N, SPR_EVAL_EDGES), rows, b), dim3(THREADS), 0, st, s);
        hipLaunchKernelGGL(k_bme_spr_move, dim3(1, b), dim3(THREADS), 0, st, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// asynchronous on `st`: q and the lengths of the final topologies
inline hipError_t launch_spr_finish(hipStream_t st, const SprArgs& s, int B) {
    hipLaunchKernelGGL(k_bme_eval, dim3((unsigned)s.b.part_cap, (unsigned)B), dim3(THREADS), 0, st, s.b);
    return launch_lengths(st, s.b, B);
}

}  // namespace pfbme
