// Least-squares branch lengths on the device (pf_tree_ols, pf_tree_ols_device): float preds [B][P_N], join
// tables slots int32 [B][M][T] -> ols double [B][M][T], status uint8 [B][M], bit for bit those of pf_ols_host.h::run_serial and of
// ols.py::tree_ols_py.  The arithmetic is pf_ols_host.h's; this file is the kernels and their launches.  An item is one tree of
// one source, item = source * M + tree.
//   k_fit_scan      pf_fit.hip.h's: a NaN or an infinity among a source's distances sets the source's word of the chunk's flags
//   k_ols_setup     one workgroup per item: replays the table in LDS with pf_fit_host.h::replay's checks and sets the status; one
//                   thread names the node behind every entry (kids), counts the leaves below every node in ascending order and
//                   places every node in the leaf order in descending order - the serial part -; all threads then store kids,
//                   cnt, lo and ord of the item
//   k_ols_columns   one thread per (item, leaf x): column x of W - the leaves' rows from preds, then the joins in their order,
//                   then r - in the item's [node][x] array; consecutive threads take consecutive x, so the stores and the loads
//                   of W coalesce, and a column needs nothing from another: no synchronisation
//   k_ols_branches  one wave per (item, branch): lane l is accumulator l of the statement's six group sums, the lanes are combined
//                   by shuffles in the statement's order, lane 0 evaluates the closed form and stores ols[k]
// An item with a status is walked by no kernel after the setup; its results are the zeros the launch starts with.  The one
// atomic is k_fit_scan's integer OR; no floating-point value is shared between workgroups: one call with B sources equals B
// calls with one.  There is no size switch: the setup's LDS - 16 bytes a sequence - holds the cap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_fit.hip.h"
#include "pf_ols_host.h"

namespace pfols {

constexpr int SETUP_THREADS = 256, COLUMN_THREADS = 256, BRANCH_THREADS = 256;
// k_ols_setup's LDS: kids [T] and one int32 per node (the slots' nodes, then cnt, then lo): 131,052 bytes at the cap
constexpr int SETUP_LDS_MAX = (table_len(MAX_N) + nodes_of(MAX_N)) * (int)sizeof(int32_t);

struct Args {
    const float* preds;        // [B][P]
    const int32_t* slots;      // [B][M][T]
    double* ols;               // [B][M][T]
    uint8_t* status;           // [B][M]
    double* W;                 // the chunk's [nb][2N - 2][N]
    unsigned int* bad_source;  // the chunk's [nb] (two words each): source src0 + k holds a NaN or an infinity
    int32_t* cnt;              // the chunk's [nb][2N - 2]
    int32_t* kids;             // the chunk's [nb][T]
    int32_t* lo;               // the chunk's [nb][2N - 2]
    int32_t* ord;              // the chunk's [nb][N]
    int64_t src0;              // the first source of the chunk
    int64_t P;
    int64_t item0;
    int nb, N, M, gx;          // gx: workgroups of k_ols_columns per item
};

// the chunk's arrays, one list for their bytes and their places (pf_spans.h)
template <class V>
inline void state_arrays(V& v, Args& a, size_t nb, int N) {
    const size_t nodes = (size_t)nodes_of(N), n = (size_t)N;
    v(a.W, nb * nodes * n);
    v(a.bad_source, nb * 2);
    v(a.cnt, nb * nodes);
    v(a.kids, nb * (size_t)table_len(N));
    v(a.lo, nb * nodes);
    v(a.ord, nb * n);
}
// the workspace of one item of a chunk: nb items take nb times that at the most
inline size_t state_bytes(int N) {
    Args a{};
    return pfspan::measure([&](auto& v) { state_arrays(v, a, 1, N); });
}
inline void carve(Args& a, char* base, int nb) {
    pfspan::carve(base, [&](auto& v) { state_arrays(v, a, (size_t)nb, a.N); });
}

__global__ __launch_bounds__(SETUP_THREADS) void k_ols_setup(Args a) {
    extern __shared__ __align__(8) int32_t ols_setup_lds[];      // kids [T]; u [2N - 2]: the node in every slot, then cnt, then lo
    const int tid = (int)threadIdx.x, N = a.N, T = table_len(N), nodes = nodes_of(N);
    const int64_t item = a.item0 + (int64_t)blockIdx.x, src = item / a.M;
    const int32_t* sl = a.slots + (size_t)item * (size_t)T;
    int32_t* kids = ols_setup_lds;
    int32_t* u = ols_setup_lds + T;
    const int bad = a.bad_source[src - a.src0] ? 1 : 0;
    for (int k = tid; k < T; k += SETUP_THREADS) kids[k] = sl[k];
    __syncthreads();
    __shared__ int no_table;
    if (tid == 0) {
        const int wrong = replay_kids(kids, N, u, kids) != OK;
        no_table = wrong;
        a.status[item] = wrong ? NO_TABLE : (bad ? NONFINITE : OK);
    }
    __syncthreads();
    if (no_table || bad) return;
    for (int v = tid; v < nodes; v += SETUP_THREADS) u[v] = 1;
    __syncthreads();
    if (tid == 0) count_leaves(kids, N, u);
    __syncthreads();
    int32_t* g_kids = a.kids + (size_t)blockIdx.x * (size_t)T;
    int32_t* g_cnt = a.cnt + (size_t)blockIdx.x * (size_t)nodes;
    int32_t* g_lo = a.lo + (size_t)blockIdx.x * (size_t)nodes;
    int32_t* g_ord = a.ord + (size_t)blockIdx.x * (size_t)N;
    for (int k = tid; k < T; k += SETUP_THREADS) g_kids[k] = kids[k];
    for (int v = tid; v < nodes; v += SETUP_THREADS) g_cnt[v] = u[v];
    __syncthreads();
    if (tid == 0) leaf_offsets(kids, N, u, u);
    __syncthreads();
    for (int v = tid; v < nodes; v += SETUP_THREADS) g_lo[v] = u[v];
    for (int x = tid; x < N; x += SETUP_THREADS) g_ord[u[x]] = x;      // (the leaves' offsets are a permutation of 0 .. N-1)
}

__global__ __launch_bounds__(COLUMN_THREADS) void k_ols_columns(Args a) {
    const int N = a.N;
    const int64_t local = (int64_t)blockIdx.x / a.gx;
    const int x = (int)((int64_t)blockIdx.x - local * a.gx) * COLUMN_THREADS + (int)threadIdx.x;
    const int64_t item = a.item0 + local;
    if (x >= N || a.status[item]) return;
    column(a.preds + (size_t)(item / a.M) * (size_t)a.P, a.kids + (size_t)local * (size_t)table_len(N), N, x,
           a.W + (size_t)local * (size_t)nodes_of(N) * (size_t)N);
}

__global__ __launch_bounds__(BRANCH_THREADS) void k_ols_branches(Args a) {
    const int lane = (int)threadIdx.x & 63, N = a.N, T = table_len(N), nodes = nodes_of(N);
    const int64_t w = (int64_t)blockIdx.x * (BRANCH_THREADS / 64) + ((int)threadIdx.x >> 6);      // (local item, branch)
    if (w >= (int64_t)a.nb * T) return;
    const int64_t local = w / T, item = a.item0 + local;
    const int k = (int)(w - local * T);
    if (a.status[item]) return;
    const double* W = a.W + (size_t)local * (size_t)nodes * (size_t)N;
    const int32_t* kids = a.kids + (size_t)local * (size_t)T;
    const int32_t* cnt = a.cnt + (size_t)local * (size_t)nodes;
    const Branch br = branch_of(kids, cnt, N, k);
    Part p = branch_lane(W, N, kids, cnt, a.lo + (size_t)local * (size_t)nodes, a.ord + (size_t)local * (size_t)N, br, lane);
    for (int s = 32; s > 0; s >>= 1) {
        Part o;
        o.cd = __shfl_down(p.cd, s, 64); o.ab = __shfl_down(p.ab, s, 64); o.ac = __shfl_down(p.ac, s, 64);
        o.bc = __shfl_down(p.bc, s, 64); o.ad = __shfl_down(p.ad, s, 64); o.bd = __shfl_down(p.bd, s, 64);
        if (lane < s) part_merge(p, o);
    }
    if (lane == 0) a.ols[(size_t)item * (size_t)T + k] = branch_length(W, N, kids, cnt, br, p);
}

// The kernels of one chunk - items item0 .. item0 + nb of the call, carved - asynchronous on `s`.
inline hipError_t launch_chunk(hipStream_t s, Args a) {
    const int N = a.N, T = table_len(N);
    a.src0 = a.item0 / a.M;
    const int64_t sources = (a.item0 + a.nb - 1) / a.M - a.src0 + 1;      // <= nb
    hipError_t e = hipMemsetAsync(a.bad_source, 0, (size_t)sources * sizeof(unsigned int), s);
    if (e != hipSuccess) return e;
    pffit::Args scan{};
    scan.preds = a.preds; scan.bad_source = a.bad_source; scan.src0 = a.src0; scan.P = a.P;
    scan.scan_groups = (int)std::max<int64_t>(1, std::min<int64_t>(pffit::SCAN_GROUPS, a.P / (pffit::SCAN_THREADS * pffit::SCAN_PER_THREAD)));
    hipLaunchKernelGGL(pffit::k_fit_scan, dim3((unsigned)(sources * scan.scan_groups)), dim3(pffit::SCAN_THREADS), 0, s, scan);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ols_setup, dim3((unsigned)a.nb), dim3(SETUP_THREADS), (size_t)(T + nodes_of(N)) * sizeof(int32_t), s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    a.gx = (N + COLUMN_THREADS - 1) / COLUMN_THREADS;
    hipLaunchKernelGGL(k_ols_columns, dim3((unsigned)((int64_t)a.nb * a.gx)), dim3(COLUMN_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t waves = (int64_t)a.nb * T;
    hipLaunchKernelGGL(k_ols_branches, dim3((unsigned)((waves + BRANCH_THREADS / 64 - 1) / (BRANCH_THREADS / 64))), dim3(BRANCH_THREADS), 0, s, a);
    return hipGetLastError();
}

// the items of one chunk at the most: the grids stay below 2^31 blocks
inline int64_t max_items(int N) { return std::max<int64_t>(1, ((int64_t)1 << 30) / std::max(2 * N, pffit::SCAN_GROUPS)); }

}  // namespace pfols
