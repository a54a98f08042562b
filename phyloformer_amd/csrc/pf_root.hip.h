// Tree rooting on the device (pf_tree_root, pf_tree_root_device): join tables slots int32 / lengths double
// [B][M][T] -> ssq, pos double [B][M][T], mid double [B][M][5], status uint8 [B][M], bit for bit those of
// pf_root_host.h::run_serial and of root.py::tree_root_py.  The arithmetic is pf_root_host.h's; this file is the kernels and their
// launches.  An item is one tree, item = source * M + tree.
//   k_root_scan      one workgroup per item: a NaN or an infinity among the item's lengths sets the item's word of the flags
//   k_ols_setup      pf_ols.hip.h's, every item a source of its own: replay with pf_fit_host.h::replay's checks, the status, kids,
//                    cnt, lo and ord of the item
//   k_root_nodes     one thread per (item, entry): the parent and the clamped length of the node behind the entry
//   k_root_columns   one thread per (item, place q): column q of D; consecutive threads take consecutive q, so the stores and the
//                    loads coalesce, and a column needs nothing from another
//   k_root_weights   one thread per (item, c, q): Wt[c][q]
//   k_root_position  one wave per (item, entry): lane l is accumulator l of the two position sums, combined by shuffles in the
//                    statement's order; lane 0 stores pos[k]
//   k_root_score     the hot path.  A workgroup of four waves owns 16 entries, four a wave, and walks the places in groups of 256
//                    and the partners c in chunks of 256.  Per chunk the 16 x 256 root-to-tip distances t_k[c] are staged in LDS
//                    (every lane of a wave reads the same address: a broadcast); a thread holds 4 entries x 4 places in registers,
//                    so one load of Wt and one LDS read of t_k[c] serve four terms each.  Lane l takes the places q = l (mod 64)
//                    ascending and adds each finished row sum to its accumulator; the 64 accumulators are combined by shuffles:
//                    no row sum goes to memory
//   k_root_far       one wave per (item, leaf c): the farthest leaf b < c of row c
//   k_root_mid       one workgroup per item: the farthest pair of all rows, then the first entry whose branch holds the midpoint
// An item with a status is walked by no kernel after the setup; its results are the zeros the launch starts with.  No
// floating-point value is shared between workgroups by an atomic: one call with B sources equals B calls with one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_ols.hip.h"
#include "pf_root_host.h"

namespace pfroot {

constexpr int THREADS = 256;
constexpr int SCORE_K = 4, SCORE_Q = 4;                    // entries and places a thread of k_root_score holds
constexpr int SCORE_ENTRIES = SCORE_K * (THREADS / 64);    // entries a workgroup owns: 16
constexpr int SCORE_PLACES = SCORE_Q * 64;                 // places of one group: 256
constexpr int SCORE_CHUNK = 256;                           // partners c staged at a time: 16 x 256 doubles = 32 KiB of LDS

struct Args {
    const int32_t* slots;      // [B][M][T]
    const double* lengths;     // [B][M][T]
    double* ssq;               // [B][M][T]
    double* pos;               // [B][M][T]
    double* mid;               // [B][M][5]
    uint8_t* status;           // [B][M]
    double* D;                 // the chunk's [nb][2N - 2][N]
    double* Wt;                // the chunk's [nb][N][N]
    double* L;                 // the chunk's [nb][2N - 2]
    double* far_d;             // the chunk's [nb][N]: row c's farthest D[c][b], b < c
    unsigned int* bad;         // the chunk's [nb]: the item holds a NaN or an infinity
    int32_t* cnt;              // the chunk's [nb][2N - 2]
    int32_t* kids;             // the chunk's [nb][T]
    int32_t* lo;               // the chunk's [nb][2N - 2]
    int32_t* ord;              // the chunk's [nb][N]
    int32_t* parent;           // the chunk's [nb][2N - 2]
    int32_t* far_b;            // the chunk's [nb][N]
    int64_t item0;
    int nb, N, gx;             // gx: workgroups per row of N places
};

// the chunk's arrays, one list for their bytes and their places (pf_spans.h)
template <class V>
inline void state_arrays(V& v, Args& a, size_t nb, int N) {
    const size_t nodes = (size_t)nodes_of(N), n = (size_t)N;
    v(a.D, nb * nodes * n);
    v(a.Wt, nb * n * n);
    v(a.L, nb * nodes);
    v(a.far_d, nb * n);
    v(a.bad, nb);
    v(a.cnt, nb * nodes);
    v(a.kids, nb * (size_t)table_len(N));
    v(a.lo, nb * nodes);
    v(a.ord, nb * n);
    v(a.parent, nb * nodes);
    v(a.far_b, nb * n);
}
// the workspace of one item of a chunk: nb items take nb times that at the most
inline size_t state_bytes(int N) {
    Args a{};
    return pfspan::measure([&](auto& v) { state_arrays(v, a, 1, N); });
}
inline void carve(Args& a, char* base, int nb) {
    pfspan::carve(base, [&](auto& v) { state_arrays(v, a, (size_t)nb, a.N); });
}

__global__ __launch_bounds__(THREADS) void k_root_scan(Args a) {
    const int T = table_len(a.N);
    const double* len = a.lengths + (size_t)(a.item0 + (int64_t)blockIdx.x) * (size_t)T;
    bool bad = false;
    for (int k = (int)threadIdx.x; k < T; k += THREADS) bad |= pffit::nonfinite(len[k]);
    if (bad) atomicOr(a.bad + blockIdx.x, 1u);
}

__global__ __launch_bounds__(THREADS) void k_root_nodes(Args a) {
    const int N = a.N, T = table_len(N), nodes = nodes_of(N);
    const int64_t local = (int64_t)blockIdx.x / a.gx;
    const int k = (int)((int64_t)blockIdx.x - local * a.gx) * THREADS + (int)threadIdx.x;
    const int64_t item = a.item0 + local;
    if (k >= T || a.status[item]) return;
    int32_t* parent = a.parent + (size_t)local * (size_t)nodes;
    double* L = a.L + (size_t)local * (size_t)nodes;
    node_of_entry(a.kids + (size_t)local * (size_t)T, a.lengths + (size_t)item * (size_t)T, N, k, parent, L);
    if (k == 0) { parent[nodes - 1] = nodes - 1; L[nodes - 1] = 0.0; }
}

__global__ __launch_bounds__(THREADS) void k_root_columns(Args a) {
    const int N = a.N, nodes = nodes_of(N);
    const int64_t local = (int64_t)blockIdx.x / a.gx;
    const int q = (int)((int64_t)blockIdx.x - local * a.gx) * THREADS + (int)threadIdx.x;
    if (q >= N || a.status[a.item0 + local]) return;
    column(a.parent + (size_t)local * (size_t)nodes, a.L + (size_t)local * (size_t)nodes, a.cnt + (size_t)local * (size_t)nodes,
           a.lo + (size_t)local * (size_t)nodes, N, q, a.ord[(size_t)local * (size_t)N + q], a.D + (size_t)local * (size_t)nodes * (size_t)N);
}

__global__ __launch_bounds__(THREADS) void k_root_weights(Args a) {
    const int N = a.N;
    const int64_t row = (int64_t)blockIdx.x / a.gx, local = row / N;
    const int c = (int)(row - local * N);
    const int q = (int)((int64_t)blockIdx.x - row * a.gx) * THREADS + (int)threadIdx.x;
    if (q >= N || a.status[a.item0 + local]) return;
    const double* D = a.D + (size_t)local * (size_t)nodes_of(N) * (size_t)N;
    const int x = a.ord[(size_t)local * (size_t)N + q];
    a.Wt[((size_t)local * (size_t)N + (size_t)c) * (size_t)N + q] = weight(D[(size_t)x * (size_t)N + c]);
}

__global__ __launch_bounds__(THREADS) void k_root_position(Args a) {
    const int lane = (int)threadIdx.x & 63, N = a.N, T = table_len(N), nodes = nodes_of(N);
    const int64_t w = (int64_t)blockIdx.x * (THREADS / 64) + ((int)threadIdx.x >> 6);      // (local item, entry)
    if (w >= (int64_t)a.nb * T) return;
    const int64_t local = w / T, item = a.item0 + local;
    const int k = (int)(w - local * T);
    if (a.status[item]) return;
    const int v = a.kids[(size_t)local * (size_t)T + k];
    const int lo_v = a.lo[(size_t)local * (size_t)nodes + v], n_v = a.cnt[(size_t)local * (size_t)nodes + v];
    Part p = position_lane(a.D + (size_t)local * (size_t)nodes * (size_t)N, a.Wt + (size_t)local * (size_t)N * (size_t)N, N, v, lo_v, n_v, lane);
    for (int s = 32; s > 0; s >>= 1) {
        Part o;
        o.s1 = __shfl_down(p.s1, s, 64); o.s0 = __shfl_down(p.s0, s, 64);
        if (lane < s) part_merge(p, o);
    }
    if (lane == 0) a.pos[(size_t)item * (size_t)T + k] = position(p, a.L[(size_t)local * (size_t)nodes + v]);
}

__global__ __launch_bounds__(THREADS) void k_root_score(Args a) {
#pragma clang fp contract(off)
    __shared__ double t_c[SCORE_ENTRIES][SCORE_CHUNK];
    __shared__ double s_lam[SCORE_ENTRIES];
    __shared__ int s_v[SCORE_ENTRIES], s_lo[SCORE_ENTRIES], s_n[SCORE_ENTRIES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N, T = table_len(N), nodes = nodes_of(N);
    const int64_t local = (int64_t)blockIdx.x / a.gx, item = a.item0 + local;      // (gx: workgroups per item here)
    const int k0 = (int)((int64_t)blockIdx.x - local * a.gx) * SCORE_ENTRIES;
    if (a.status[item]) return;                                                    // (the whole workgroup)
    const size_t n = (size_t)N;
    const double* D = a.D + (size_t)local * (size_t)nodes * n;
    const double* Wt = a.Wt + (size_t)local * n * n;
    if (tid < SCORE_ENTRIES) {
        const int k = std::min(k0 + tid, T - 1);       // (an entry past the table repeats the last one and stores nothing)
        const int v = a.kids[(size_t)local * (size_t)T + k];
        s_v[tid] = v;
        s_lo[tid] = a.lo[(size_t)local * (size_t)nodes + v];
        s_n[tid] = a.cnt[(size_t)local * (size_t)nodes + v];
        s_lam[tid] = a.pos[(size_t)item * (size_t)T + k];
    }
    __syncthreads();
    const int e0 = wave * SCORE_K;
    double acc[SCORE_K];
#pragma unroll
    for (int i = 0; i < SCORE_K; ++i) acc[i] = 0.0;
    for (int q0 = 0; q0 < N; q0 += SCORE_PLACES) {
        int q[SCORE_Q];
        double t_q[SCORE_K][SCORE_Q], r[SCORE_K][SCORE_Q];
#pragma unroll
        for (int j = 0; j < SCORE_Q; ++j) q[j] = std::min(q0 + 64 * j + lane, N - 1);      // (a place past the end is not added)
#pragma unroll
        for (int i = 0; i < SCORE_K; ++i)
#pragma unroll
            for (int j = 0; j < SCORE_Q; ++j) {
                t_q[i][j] = tip(D[(size_t)s_v[e0 + i] * n + q[j]], s_lam[e0 + i], below(s_lo[e0 + i], s_n[e0 + i], q[j]));
                r[i][j] = 0.0;
            }
        for (int c0 = 0; c0 < N; c0 += SCORE_CHUNK) {
            __syncthreads();                           // the chunk before has been read
            if (c0 + tid < N)
                for (int e = 0; e < SCORE_ENTRIES; ++e)
                    t_c[e][tid] = tip(D[(size_t)s_v[e] * n + c0 + tid], s_lam[e], below(s_lo[e], s_n[e], c0 + tid));
            __syncthreads();
            const int span = std::min(SCORE_CHUNK, N - c0);
            for (int cc = 0; cc < span; ++cc) {
                const double* row = Wt + (size_t)(c0 + cc) * n;
                double w[SCORE_Q];
#pragma unroll
                for (int j = 0; j < SCORE_Q; ++j) w[j] = row[q[j]];
#pragma unroll
                for (int i = 0; i < SCORE_K; ++i) {
                    const double tc = t_c[e0 + i][cc];
#pragma unroll
                    for (int j = 0; j < SCORE_Q; ++j) r[i][j] = r[i][j] + term(w[j], t_q[i][j], tc);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SCORE_Q; ++j)
            if (q0 + 64 * j + lane < N) {
#pragma unroll
                for (int i = 0; i < SCORE_K; ++i) acc[i] = acc[i] + r[i][j];
            }
    }
#pragma unroll
    for (int i = 0; i < SCORE_K; ++i) {
        double s = acc[i];
        for (int d = 32; d > 0; d >>= 1) {
            const double o = __shfl_down(s, d, 64);
            if (lane < d) s = s + o;
        }
        const int k = k0 + e0 + i;
        if (lane == 0 && k < T) a.ssq[(size_t)item * (size_t)T + k] = 0.5 * s;
    }
}

__global__ __launch_bounds__(THREADS) void k_root_far(Args a) {
    const int lane = (int)threadIdx.x & 63, N = a.N, nodes = nodes_of(N);
    const int64_t w = (int64_t)blockIdx.x * (THREADS / 64) + ((int)threadIdx.x >> 6);      // (local item, leaf c)
    if (w >= (int64_t)a.nb * N) return;
    const int64_t local = w / N;
    const int c = (int)(w - local * N);
    if (a.status[a.item0 + local]) return;
    const double* row = a.D + ((size_t)local * (size_t)nodes + (size_t)c) * (size_t)N;
    const int32_t* ord = a.ord + (size_t)local * (size_t)N;
    Far f = far_none();
    for (int q = lane; q < N; q += 64) {
        const int b = ord[q];
        if (b < c) far_take(f, Far{row[q], b, c});
    }
    for (int s = 32; s > 0; s >>= 1) {
        Far o;
        o.d = __shfl_down(f.d, s, 64); o.b = __shfl_down(f.b, s, 64); o.c = c;
        if (lane < s) far_take(f, o);
    }
    if (lane == 0) { a.far_d[(size_t)local * (size_t)N + c] = f.d; a.far_b[(size_t)local * (size_t)N + c] = f.b; }
}

__global__ __launch_bounds__(THREADS) void k_root_mid(Args a) {
    __shared__ double s_d[THREADS];
    __shared__ int s_b[THREADS], s_c[THREADS];
    __shared__ int first;
    const int tid = (int)threadIdx.x, N = a.N, T = table_len(N), nodes = nodes_of(N);
    const int64_t local = blockIdx.x, item = a.item0 + local;
    if (a.status[item]) return;
    Far f = far_none();
    for (int c = 1 + tid; c < N; c += THREADS) far_take(f, Far{a.far_d[(size_t)local * (size_t)N + c], a.far_b[(size_t)local * (size_t)N + c], c});
    s_d[tid] = f.d; s_b[tid] = f.b; s_c[tid] = f.c;
    if (tid == 0) first = T;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            far_take(f, Far{s_d[tid + s], s_b[tid + s], s_c[tid + s]});
            s_d[tid] = f.d; s_b[tid] = f.b; s_c[tid] = f.c;
        }
        __syncthreads();
    }
    f = Far{s_d[0], s_b[0], s_c[0]};
    const double half = 0.5 * f.d;
    const double* D = a.D + (size_t)local * (size_t)nodes * (size_t)N;
    const int32_t* kids = a.kids + (size_t)local * (size_t)T;
    const int32_t* parent = a.parent + (size_t)local * (size_t)nodes;
    const int32_t* cnt = a.cnt + (size_t)local * (size_t)nodes;
    const int32_t* lo = a.lo + (size_t)local * (size_t)nodes;
    double lam = 0.0;
    for (int k = tid; k < T; k += THREADS)
        if (mid_entry(D, kids, parent, cnt, lo, N, k, f.b, f.c, half, &lam)) { atomicMin(&first, k); break; }
    __syncthreads();
    const int k = first;
    if (k < T && k % THREADS == tid) {                 // (the thread that walked entry k; its first hit is k itself)
        double* mid = a.mid + (size_t)item * MID;
        mid_entry(D, kids, parent, cnt, lo, N, k, f.b, f.c, half, &lam);
        mid[0] = (double)k; mid[1] = lam; mid[2] = (double)f.b; mid[3] = (double)f.c; mid[4] = f.d;
    }
}

// The kernels of one chunk - items item0 .. item0 + nb of the call, carved - asynchronous on `s`.
inline hipError_t launch_chunk(hipStream_t s, Args a) {
    const int N = a.N, T = table_len(N);
    const int64_t nb = a.nb;
    hipError_t e = hipMemsetAsync(a.bad, 0, (size_t)nb * sizeof(unsigned int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_root_scan, dim3((unsigned)nb), dim3(THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    pfols::Args o{};      // every item a source of its own
    o.slots = a.slots; o.status = a.status; o.bad_source = a.bad; o.cnt = a.cnt; o.kids = a.kids; o.lo = a.lo; o.ord = a.ord;
    o.src0 = a.item0; o.item0 = a.item0; o.nb = a.nb; o.N = N; o.M = 1;
    hipLaunchKernelGGL(pfols::k_ols_setup, dim3((unsigned)nb), dim3(pfols::SETUP_THREADS), (size_t)(T + nodes_of(N)) * sizeof(int32_t), s, o);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    a.gx = (T + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(k_root_nodes, dim3((unsigned)(nb * a.gx)), dim3(THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    a.gx = (N + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(k_root_columns, dim3((unsigned)(nb * a.gx)), dim3(THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_root_weights, dim3((unsigned)(nb * N * a.gx)), dim3(THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t waves = nb * T, per = THREADS / 64;
    hipLaunchKernelGGL(k_root_position, dim3((unsigned)((waves + per - 1) / per)), dim3(THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    a.gx = (T + SCORE_ENTRIES - 1) / SCORE_ENTRIES;
    hipLaunchKernelGGL(k_root_score, dim3((unsigned)(nb * a.gx)), dim3(THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_root_far, dim3((unsigned)((nb * N + per - 1) / per)), dim3(THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_root_mid, dim3((unsigned)nb), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

// the items of one chunk at the most: the grids stay below 2^31 blocks
inline int64_t max_items(int N) { return std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)N * ((N + THREADS - 1) / THREADS))); }

}  // namespace pfroot
