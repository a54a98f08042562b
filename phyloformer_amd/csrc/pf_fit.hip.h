// Tree fit on the device (pf_tree_fit, pf_tree_fit_device): float preds [B][P_N], join tables slots int32 /
// lengths double [B][M][T] -> patristic double [B][M][P_N] (or none), rows double [B][M][N][6], worst_j int32 [B][M][N], status
// uint8 [B][M], bit for bit those of pf_fit_host.h::run_serial and of fit.py::tree_fit_py.  The arithmetic is pf_fit_host.h's;
// this file is the kernels and their launches.  An item is one tree of one source, item = source * M + tree.
//   k_fit_scan   up to SCAN_GROUPS workgroups per source of the chunk: a NaN or an infinity among its distances sets the
//                source's word of the chunk's flags (an integer OR: no order shows)
//   k_fit_setup  one workgroup per item: takes its source's flag, looks for a NaN or an infinity among the tree's lengths, replays
//                the table in LDS - one thread names the node in every entry of the table, which is the serial part; all
//                threads then store parent / len [2N - 2] of the item - and sets the status
//   k_fit_pairs  G workgroups per item: the node arrays staged in LDS (template LDS = true, up to LDS_MAX_BYTES) or read from
//                global memory; workgroup g takes the rows x = g, g + G, ... of the triangle, its threads consecutive y, so
//                the stores of T coalesce; each pair is pf_fit_host.h::walk
//   k_fit_rows   one wave per (item, sequence): lane l is accumulator l of the statement, the lanes are combined by shuffles
//                in the statement's order
// An item with a status is walked by no kernel; its results are the zeros the launch starts with.  The one atomic is k_fit_scan's
// integer OR; no floating-point value is shared between workgroups: one call with B sources equals B calls with one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_fit_host.h"

namespace pffit {

constexpr int SETUP_THREADS = 256, PAIR_THREADS = 1024, ROW_THREADS = 256, SCAN_THREADS = 256;
constexpr int SCAN_GROUPS = 256, SCAN_PER_THREAD = 16;      // a source's distances: 16 a thread at the least, 256 workgroups at the most
// the LDS of a CU (gfx950): the node arrays of a tree, 12 bytes a node, are staged where they fit - N <= 6,827
constexpr int LDS_MAX_BYTES = 160 * 1024;
constexpr int NODE_BYTES = (int)(sizeof(double) + sizeof(int32_t));
constexpr int SETUP_LDS_MAX = (table_len(MAX_N) + MAX_N) * (int)sizeof(int32_t);      // 98,292 bytes at the cap
constexpr int PAIR_GROUPS = 1024;          // workgroups of k_fit_pairs a chunk aims for (four a CU), one per item at the least

struct Args {
    const float* preds;        // [B][P]
    const int32_t* slots;      // [B][M][T]
    const double* lengths;     // [B][M][T]
    double* tree;              // T of item `item0`, [nb][P]: the caller's patristic or the chunk's workspace
    double* rows;              // [B][M][N][6]
    int32_t* worst_j;          // [B][M][N]
    uint8_t* status;           // [B][M]
    int32_t* parent;           // the chunk's [nb][2N - 2]
    double* len;               // the chunk's [nb][2N - 2]
    unsigned int* bad_source;  // the chunk's [nb]: source src0 + k holds a NaN or an infinity (zeroed before k_fit_scan)
    int64_t src0;              // the first source of the chunk
    int scan_groups;           // workgroups of k_fit_scan per source
    int64_t P;
    int64_t item0;
    int nb, N, M, G;
};

// the workspace of one item of a chunk: its node arrays and, without the caller's patristic, its T
inline size_t state_bytes(int N, bool own_tree) {
    const size_t n = (size_t)N;
    return (size_t)nodes_of(N) * 16 + 8 + (own_tree ? n * (n - 1) / 2 * sizeof(double) : 0);
}

// the chunk's arrays from `base` (8-byte aligned): len, tree, the sources' flags, parent
inline void carve(Args& a, char* base, int nb, bool own_tree) {
    const size_t nodes = (size_t)nodes_of(a.N);
    a.len = reinterpret_cast<double*>(base);
    base += (size_t)nb * nodes * sizeof(double);
    if (own_tree) { a.tree = reinterpret_cast<double*>(base); base += (size_t)nb * (size_t)a.P * sizeof(double); }
    a.bad_source = reinterpret_cast<unsigned int*>(base);
    base += (size_t)nb * 8;
    a.parent = reinterpret_cast<int32_t*>(base);
}

__global__ __launch_bounds__(SCAN_THREADS) void k_fit_scan(Args a) {
    const int64_t local = (int64_t)blockIdx.x / a.scan_groups;
    const int g = (int)((int64_t)blockIdx.x - local * a.scan_groups);
    const float* pr = a.preds + (size_t)(a.src0 + local) * (size_t)a.P;
    int bad = 0;
    for (int64_t e = (int64_t)g * SCAN_THREADS + threadIdx.x; e < a.P; e += (int64_t)a.scan_groups * SCAN_THREADS)
        bad |= nonfinite((double)pr[e]) ? 1 : 0;
    bad = __syncthreads_or(bad);
    if (bad && threadIdx.x == 0) atomicOr(&a.bad_source[local], 1u);
}

__global__ __launch_bounds__(SETUP_THREADS) void k_fit_setup(Args a) {
    extern __shared__ __align__(8) int32_t setup_lds[];      // the table's T slots - then the node of every entry -, N nodes
    const int tid = (int)threadIdx.x, N = a.N, T = table_len(N), J = N - 3;
    const int64_t item = a.item0 + (int64_t)blockIdx.x, src = item / a.M;
    const int32_t* sl = a.slots + (size_t)item * (size_t)T;
    const double* ln = a.lengths + (size_t)item * (size_t)T;
    int32_t* entry = setup_lds;
    int32_t* node = setup_lds + T;
    int bad = a.bad_source[src - a.src0] ? 1 : 0;
    for (int k = tid; k < T; k += SETUP_THREADS) { bad |= nonfinite(ln[k]) ? 1 : 0; entry[k] = sl[k]; }
    for (int s = tid; s < N; s += SETUP_THREADS) node[s] = s;
    bad = __syncthreads_or(bad);
    __shared__ int no_table;
    if (tid == 0) {
        // pf_fit_host.h::replay's checks; entry[k] becomes the node that entry k of the table names
        int wrong = 0;
        for (int t = 0; t < J && !wrong; ++t) {
            const int32_t x = entry[2 * t], y = entry[2 * t + 1];
            if (x < 0 || x >= N || y < 0 || y >= N || x == y || node[x] < 0 || node[y] < 0) { wrong = 1; break; }
            entry[2 * t] = node[x]; entry[2 * t + 1] = node[y];
            node[x] = N + t; node[y] = -1;
        }
        for (int k = 0; k < 3 && !wrong; ++k) {
            const int32_t s = entry[2 * J + k];
            if (s < 0 || s >= N || node[s] < 0) { wrong = 1; break; }
            entry[2 * J + k] = node[s];
            node[s] = -1;
        }
        no_table = wrong;
        a.status[item] = wrong ? NO_TABLE : (bad ? NONFINITE : OK);
    }
    __syncthreads();
    if (no_table || bad) return;
    const int nodes = nodes_of(N), root = 2 * N - 3;
    int32_t* parent = a.parent + (size_t)blockIdx.x * (size_t)nodes;
    double* len = a.len + (size_t)blockIdx.x * (size_t)nodes;
    for (int k = tid; k < T; k += SETUP_THREADS) {           // every node but the last is named by exactly one entry
        const int c = entry[k];
        parent[c] = k < 2 * J ? N + (k >> 1) : root;
        len[c] = ln[k];
    }
    if (tid == 0) { parent[root] = root; len[root] = 0.0; }
}

template <bool LDS>
__global__ __launch_bounds__(PAIR_THREADS) void k_fit_pairs(Args a) {
    extern __shared__ __align__(8) double pair_lds[];        // LDS: len [2N - 2], then parent [2N - 2]
    const int tid = (int)threadIdx.x, N = a.N, nodes = nodes_of(N);
    const int64_t local = (int64_t)blockIdx.x / a.G;
    const int g = (int)((int64_t)blockIdx.x - local * a.G);
    if (a.status[a.item0 + local]) return;
    const int32_t* parent = a.parent + (size_t)local * (size_t)nodes;
    const double* len = a.len + (size_t)local * (size_t)nodes;
    if (LDS) {
        double* l_len = pair_lds;
        int32_t* l_parent = reinterpret_cast<int32_t*>(pair_lds + nodes);
        for (int k = tid; k < nodes; k += PAIR_THREADS) { l_len[k] = len[k]; l_parent[k] = parent[k]; }
        __syncthreads();
        parent = l_parent; len = l_len;
    }
    double* out = a.tree + (size_t)local * (size_t)a.P;
    for (int x = g; x < N - 1; x += a.G) {
        double* row = out + row_start(x, N) - x - 1;             // pair (x, y) at row[y]
        for (int y = x + 1 + tid; y < N; y += PAIR_THREADS) row[y] = walk(parent, len, x, y);
    }
}

__global__ __launch_bounds__(ROW_THREADS) void k_fit_rows(Args a) {
    const int lane = (int)threadIdx.x & 63, N = a.N;
    const int64_t w = (int64_t)blockIdx.x * (ROW_THREADS / 64) + ((int)threadIdx.x >> 6);      // (local item, sequence)
    if (w >= (int64_t)a.nb * N) return;
    const int64_t local = w / N, item = a.item0 + local;
    const int i = (int)(w - local * N);
    if (a.status[item]) return;
    const float* pr = a.preds + (size_t)(item / a.M) * (size_t)a.P;
    Acc acc = row_lane(pr, a.tree + (size_t)local * (size_t)a.P, N, i, lane);
    for (int s = 32; s > 0; s >>= 1) {
        Acc o;
        o.ss = __shfl_down(acc.ss, s, 64); o.fm = __shfl_down(acc.fm, s, 64); o.st = __shfl_down(acc.st, s, 64);
        o.stt = __shfl_down(acc.stt, s, 64); o.sdt = __shfl_down(acc.sdt, s, 64); o.worst = __shfl_down(acc.worst, s, 64);
        o.wj = __shfl_down(acc.wj, s, 64);
        if (lane < s) acc_merge(acc, o);
    }
    if (lane == 0) row_store(acc, a.rows + ((size_t)item * (size_t)N + (size_t)i) * COLS, a.worst_j + (size_t)item * (size_t)N + i);
}

// The kernels of one chunk - items item0 .. item0 + nb of the call, carved - asynchronous on `s`.  `lds_bytes`: what
// k_fit_pairs may stage (LDS_MAX_BYTES; option "fit_lds_bytes" lowers it for the tests).
inline hipError_t launch_chunk(hipStream_t s, Args a, int lds_bytes) {
    const int N = a.N, nodes = nodes_of(N);
    a.src0 = a.item0 / a.M;
    const int64_t sources = (a.item0 + a.nb - 1) / a.M - a.src0 + 1;      // <= nb
    hipError_t e = hipMemsetAsync(a.bad_source, 0, (size_t)sources * sizeof(unsigned int), s);
    if (e != hipSuccess) return e;
    a.scan_groups = (int)std::max<int64_t>(1, std::min<int64_t>(SCAN_GROUPS, a.P / (SCAN_THREADS * SCAN_PER_THREAD)));
    hipLaunchKernelGGL(k_fit_scan, dim3((unsigned)(sources * a.scan_groups)), dim3(SCAN_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_fit_setup, dim3((unsigned)a.nb), dim3(SETUP_THREADS), (size_t)(table_len(N) + N) * sizeof(int32_t), s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    a.G = std::max(1, std::min(N - 1, PAIR_GROUPS / a.nb));
    const dim3 grid((unsigned)((int64_t)a.nb * a.G));
    const size_t stage = (size_t)nodes * NODE_BYTES;
    if (stage <= (size_t)std::min(lds_bytes, LDS_MAX_BYTES)) hipLaunchKernelGGL(k_fit_pairs<true>, grid, dim3(PAIR_THREADS), stage, s, a);
    else hipLaunchKernelGGL(k_fit_pairs<false>, grid, dim3(PAIR_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t waves = (int64_t)a.nb * N;
    hipLaunchKernelGGL(k_fit_rows, dim3((unsigned)((waves + ROW_THREADS / 64 - 1) / (ROW_THREADS / 64))), dim3(ROW_THREADS), 0, s, a);
    return hipGetLastError();
}

// the items of one chunk at the most: the grids stay below 2^31 blocks
inline int64_t max_items(int N) { return std::max<int64_t>(1, ((int64_t)1 << 30) / std::max(N, PAIR_GROUPS)); }
static_assert(SCAN_GROUPS <= PAIR_GROUPS, "k_fit_scan's grid is bounded with k_fit_pairs'");

}  // namespace pffit
