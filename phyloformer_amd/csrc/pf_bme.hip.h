// Balanced minimum-evolution NNI refinement on the device (pf_bme_nni, pf_bme_nni_device): float
// preds [B][P_N] and start tables -> refined join tables with balanced branch lengths, bit for bit those of the serial
// run of the same bodies (pf_bme_nni_host) and, from the final from-scratch table, of bme.py.  The bodies and the case
// analysis of the update are pf_bme_host.h's, shared with the CPU; this file is the launches.  No atomics, no
// cooperative launch; the host looks at the flags once per round of ROUND_STEPS steps.
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

namespace pfbme {

constexpr int THREADS = 256;               // every workgroup
constexpr int INIT_GROUPS = 1024;
constexpr int EVAL_EDGES = 32;             // edges per workgroup of k_bme_eval: 192 sums, 64 keys
constexpr int BME_MAX_Z = 65535;           // sources per launch (grid y or z)

__global__ __launch_bounds__(THREADS) void k_bme_init(Args a) {
    init_elems(a, (size_t)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, THREADS);
}

__global__ __launch_bounds__(THREADS) void k_bme_build(Args a) {
    const int j = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (j < a.N) build_elem(a, (size_t)blockIdx.z, (int64_t)blockIdx.y, j);
}

// the workgroup's minimum of keys[0 .. THREADS) into keys[0]
__device__ inline void reduce_keys(Key* keys) {
    for (int s = pfnj::reduce_first_step(THREADS); s > 0; s >>= 1) {
        __syncthreads();
        reduce_step(keys, (int)threadIdx.x, s, THREADS);
    }
    __syncthreads();
}

__global__ __launch_bounds__(THREADS) void k_bme_eval(Args a) {
    __shared__ double lq[EVAL_EDGES * 6];
    __shared__ Key keys[THREADS];
    const size_t src = (size_t)blockIdx.y;
    eval_q_thread(a, src, (int)blockIdx.x, EVAL_EDGES, (int)threadIdx.x, THREADS, lq);
    __syncthreads();
    keys[threadIdx.x] = eval_key_thread(a, src, (int)blockIdx.x, EVAL_EDGES, (int)threadIdx.x, THREADS, lq);
    reduce_keys(keys);
    if (threadIdx.x == 0) a.part[src * (size_t)a.part_cap + blockIdx.x] = keys[0];
}

__global__ __launch_bounds__(THREADS) void k_bme_move(Args a, int G) {
    __shared__ Key keys[THREADS];
    __shared__ Move move;
    const size_t src = (size_t)blockIdx.y;
    keys[threadIdx.x] = move_thread_key(a, src, G, (int)threadIdx.x, THREADS);
    reduce_keys(keys);
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

inline int eval_groups(int N) { return (int)((root_of(N) + EVAL_EDGES - 1) / EVAL_EDGES); }

// bytes of one source's state, every array's share a multiple of 8 except the trailing bytes
struct Layout {
    size_t d, M, q, edge_len, part, move, parent, children, steps, depth, rowh, rowcase, flags, total;
    explicit Layout(int N) {
        const size_t n = (size_t)N, nodes = (size_t)nodes_of(N), rows = (size_t)rows_of(N), root = (size_t)root_of(N);
        auto up8 = [](size_t x) { return (x + 7) / 8 * 8; };
        d = n * n * sizeof(double);
        M = rows * n * sizeof(double);
        q = root * 6 * sizeof(double);
        edge_len = root * sizeof(double);
        part = (size_t)eval_groups(N) * sizeof(Key);
        move = up8(sizeof(Move));
        parent = up8(nodes * sizeof(int32_t));
        children = up8(nodes * 3 * sizeof(int32_t));
        steps = 8;
        depth = up8(rows * nodes * sizeof(int16_t));
        rowh = up8(rows * sizeof(int16_t));
        rowcase = up8(rows);
        flags = 8;                                     // done, rebuild, status: one byte each per source
        total = d + M + q + edge_len + part + move + parent + children + steps + depth + rowh + rowcase + flags;
    }
};
inline size_t state_bytes(int N) { return Layout(N).total; }

// The state of B sources carved from `ws` (8-byte aligned, B * state_bytes(N) bytes): array after array, each
// [B][its share], so that a source's rows are contiguous.  Move is padded to 8 bytes per source in the layout but the
// array itself is dense (sizeof(Move) each).
inline Args carve(char* ws, const float* preds, int B, int N) {
    const Layout l(N);
    const size_t b = (size_t)B;
    Args a{};
    a.preds = preds; a.N = N; a.part_cap = eval_groups(N); a.PN = (int64_t)N * (N - 1) / 2;
    a.d = reinterpret_cast<double*>(ws);            ws += b * l.d;
    a.M = reinterpret_cast<double*>(ws);            ws += b * l.M;
    a.q = reinterpret_cast<double*>(ws);            ws += b * l.q;
    a.edge_len = reinterpret_cast<double*>(ws);     ws += b * l.edge_len;
    a.part = reinterpret_cast<Key*>(ws);            ws += b * l.part;
    a.move = reinterpret_cast<Move*>(ws);           ws += b * l.move;
    a.parent = reinterpret_cast<int32_t*>(ws);      ws += (b * (size_t)nodes_of(N) * sizeof(int32_t) + 7) / 8 * 8;
    a.children = reinterpret_cast<int32_t*>(ws);    ws += (b * (size_t)nodes_of(N) * 3 * sizeof(int32_t) + 7) / 8 * 8;
    a.steps = reinterpret_cast<int32_t*>(ws);       ws += b * l.steps;
    a.depth = reinterpret_cast<int16_t*>(ws);       ws += (b * (size_t)rows_of(N) * (size_t)nodes_of(N) * sizeof(int16_t) + 7) / 8 * 8;
    a.rowh = reinterpret_cast<int16_t*>(ws);        ws += (b * (size_t)rows_of(N) * sizeof(int16_t) + 7) / 8 * 8;
    a.rowcase = reinterpret_cast<int8_t*>(ws);      ws += (b * (size_t)rows_of(N) + 7) / 8 * 8;
    a.done = reinterpret_cast<uint8_t*>(ws);        ws += b;
    a.rebuild = reinterpret_cast<uint8_t*>(ws);     ws += b;
    a.status = reinterpret_cast<uint8_t*>(ws);
    return a;
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

constexpr int SPR_EVAL_EDGES = THREADS;      // target edges per workgroup of k_bme_spr_eval: one per thread

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
    __shared__ SprKey keys[THREADS];
    const size_t src = (size_t)blockIdx.z;
    keys[threadIdx.x] = spr_eval_thread(s, src, (int64_t)blockIdx.y, (int)blockIdx.x, (int)threadIdx.x, THREADS);
    for (int st = pfnj::reduce_first_step(THREADS); st > 0; st >>= 1) {
        __syncthreads();
        spr_reduce_step(keys, (int)threadIdx.x, st, THREADS);
    }
    __syncthreads();
    if (threadIdx.x == 0) s.spart[src * (size_t)s.spart_cap + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = keys[0];
}

__global__ __launch_bounds__(THREADS) void k_bme_spr_move(SprArgs s) {
    __shared__ SprKey keys[THREADS];
    const size_t src = (size_t)blockIdx.y;
    keys[threadIdx.x] = spr_move_thread_key(s, src, (int)threadIdx.x, THREADS);
    for (int st = pfnj::reduce_first_step(THREADS); st > 0; st >>= 1) {
        __syncthreads();
        spr_reduce_step(keys, (int)threadIdx.x, st, THREADS);
    }
    __syncthreads();
    if (threadIdx.x == 0) spr_decide(s, src, keys[0]);
}

// bytes of one source's state: balanced NNI's arrays that the search shares (no move, rowh, rowcase), T, the partial
// minima, the numbering and the path
struct SprLayout {
    size_t d, M, q, edge_len, T, part, spart, ints, depth, flags, total;
    explicit SprLayout(int N) {
        const size_t n = (size_t)N, nodes = (size_t)nodes_of(N), rows = (size_t)rows_of(N), root = (size_t)root_of(N);
        auto up8 = [](size_t x) { return (x + 7) / 8 * 8; };
        d = n * n * sizeof(double);
        M = rows * n * sizeof(double);
        q = root * 6 * sizeof(double);
        edge_len = root * sizeof(double);
        T = rows * rows * sizeof(double);
        part = (size_t)eval_groups(N) * sizeof(Key);
        spart = rows * (size_t)spr_eval_groups(N, SPR_EVAL_EDGES) * sizeof(SprKey);
        ints = up8(nodes * sizeof(int32_t));                       // parent, tin, tout, ndepth, path: one share each; children: three
        depth = up8(rows * nodes * sizeof(int16_t));
        flags = 8;                                                 // done, rebuild, status, sdone: one byte each per source
        total = d + M + q + edge_len + T + part + spart + 8 * ints + 8 + depth + flags;      // (+ 8: steps)
    }
};
inline size_t spr_state_bytes(int N) { return SprLayout(N).total; }

// the state of B sources carved from `ws` (8-byte aligned, B * spr_state_bytes(N) bytes), array after array
inline SprArgs spr_carve(char* ws, const float* preds, int B, int N, int64_t cap) {
    const SprLayout l(N);
    const size_t b = (size_t)B, nodes = (size_t)nodes_of(N);
    auto ints = [&](size_t per) { return (b * nodes * per * sizeof(int32_t) + 7) / 8 * 8; };
    SprArgs s{};
    Args& a = s.b;
    a.preds = preds; a.N = N; a.part_cap = eval_groups(N); a.PN = (int64_t)N * (N - 1) / 2;
    s.cap = cap > 0 ? cap : step_cap(N); s.epg = SPR_EVAL_EDGES;
    s.spart_cap = (int)(rows_of(N) * spr_eval_groups(N, SPR_EVAL_EDGES));
    a.d = reinterpret_cast<double*>(ws);            ws += b * l.d;
    a.M = reinterpret_cast<double*>(ws);            ws += b * l.M;
    a.q = reinterpret_cast<double*>(ws);            ws += b * l.q;
    a.edge_len = reinterpret_cast<double*>(ws);     ws += b * l.edge_len;
    s.T = reinterpret_cast<double*>(ws);            ws += b * l.T;
    a.part = reinterpret_cast<Key*>(ws);            ws += b * l.part;
    s.spart = reinterpret_cast<SprKey*>(ws);        ws += b * l.spart;
    a.parent = reinterpret_cast<int32_t*>(ws);      ws += ints(1);
    a.children = reinterpret_cast<int32_t*>(ws);    ws += ints(3);
    s.tin = reinterpret_cast<int32_t*>(ws);         ws += ints(1);
    s.tout = reinterpret_cast<int32_t*>(ws);        ws += ints(1);
    s.ndepth = reinterpret_cast<int32_t*>(ws);      ws += ints(1);
    s.path = reinterpret_cast<int32_t*>(ws);        ws += ints(1);
    a.steps = reinterpret_cast<int32_t*>(ws);       ws += b * 8;
    a.depth = reinterpret_cast<int16_t*>(ws);       ws += (b * (size_t)rows_of(N) * nodes * sizeof(int16_t) + 7) / 8 * 8;
    a.done = reinterpret_cast<uint8_t*>(ws);        ws += b;
    a.rebuild = reinterpret_cast<uint8_t*>(ws);     ws += b;
    a.status = reinterpret_cast<uint8_t*>(ws);      ws += b;
    s.sdone = reinterpret_cast<uint8_t*>(ws);
    return s;
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
        hipLaunchKernelGGL(k_bme_spr_eval, dim3((unsigned)spr_eval_groups(N, SPR_EVAL_EDGES), rows, b), dim3(THREADS), 0, st, s);
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
