// Split supports of join tables on the device (pf_join_supports, pf_join_supports_device): the
// Felsenstein count and the transfer distance sum of every split of a reference tree over R replicate trees, bit for bit
// those of supports.py::split_supports.  The bodies are pf_support_host.h's, shared with the CPU; this file is the
// launches.  No atomics (but k_sup_moves' integer sums), no cooperative launch, no copy to the host and no synchronisation between the launches.
//   k_sup_splits  grid (trees of the chunk), one workgroup per tree (reference and replicates alike): the joins in order,
//                 every thread checking the join (the same verdict for all) and striding over the words of its row;
//                 then the normalisation, one thread per split.  A table that is no join table never indexes memory:
//                 the walk stops and the tree is flagged.
//   k_sup_match   grid (tiles of TILE reference splits, replicates, sources): the tile's reference words in LDS; every
//                 thread walks the replicate's splits j = tid, tid + 256, ..., loads each replicate word once (lanes read
//                 neighbouring addresses: the tables are word-major), xors it against the tile's words (every lane reads
//                 the same LDS address: a broadcast) and keeps one running minimum per reference; then the wave's minimum
//                 by lane shuffles and the workgroup's through LDS.  A flagged replicate writes p - 1 and reads no table.
//   k_sup_sum     one thread per (source, split): count and transfer over the chunk's replicates, ascending.
// pf_join_transfers / pf_join_transfers_device run k_sup_match<true> in k_sup_match<false>'s place -
// the same body keeping WHICH replicate split is the closest - and then
//   k_sup_moves   grid (reference splits, sources): threads own sequences; per sequence the word of the reference split
//                 in a register, then the chunk's replicates with the key read as a scalar: the word of the replicate's
//                 closest split (a wave's 64 sequences share it: one address), one bit of their xor.  The counts go to
//                 branch_moves plainly and to moves[x] by integer atomics, the only ones here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_support_host.h"

namespace pfsup {

constexpr int SPLIT_THREADS = 256;
constexpr int MATCH_THREADS = 256, MATCH_WAVES = MATCH_THREADS / 64;
constexpr int SUM_THREADS = 64;
constexpr int MOVES_THREADS = 256;
constexpr int SUP_MAX_Y = 65535;       // replicates (grid y) and sources (grid z) of one launch
constexpr int MAX_W = 256;             // words of a split at pfbme::MAX_N sequences: the tile is TILE * MAX_W * 8 = 32 KB of LDS

// Every thread of a workgroup reads the same entries of `row`, so each value is handed over as a scalar: the checks and
// the loop's exit are then scalar too, the same for the whole workgroup.
struct UniformRows {
    const int32_t* row;
    __device__ int32_t operator()(int32_t slot) const { return __builtin_amdgcn_readfirstlane(row[slot]); }
};

__global__ __launch_bounds__(SPLIT_THREADS) void k_sup_splits(Args a) {
    const int N = a.N, S = N - 3, W = words_of(N), tid = (int)threadIdx.x;
    const int src = (int)(blockIdx.x / (unsigned)(a.rc + 1)), k = (int)(blockIdx.x % (unsigned)(a.rc + 1));
    if (flagged(a, src, k)) return;                           // (the whole workgroup)
    const int32_t* slots = slots_of(a, src, k);
    uint64_t* bits = bits_of(a, src, k);
    int32_t* row = row_of(a, src, k);
    const UniformRows rows{row};
    rows_init(row, N, tid, SPLIT_THREADS);
    __syncthreads();
    // every thread walks the joins and checks them itself (the same slots, the same rows: the same verdict); thread 0
    // alone writes `row`, between two barriers
    bool ok = true;
    for (int t = 0; t < S; ++t) {
        const int32_t sa = slots[2 * t], sb = slots[2 * t + 1];
        int32_t ra = 0, rb = 0;
        if (!join_ok(rows, N, sa, sb, &ra, &rb)) { ok = false; break; }
        __syncthreads();                                       // (every thread has read the rows of sa and sb)
        if (tid == 0) { row[sa] = t; row[sb] = DEAD; }
        join_words(bits, S, W, t, sa, ra, sb, rb, tid, SPLIT_THREADS);
        __syncthreads();                                       // (row is the next join's; after the last, every row is complete)
    }
    if (ok) ok = final_ok(rows, N, slots + 2 * (size_t)S);
    if (!ok) {
        if (tid == 0) *bad_of(a, src, k) = 1;
        return;
    }
    normalise(bits, S, W, N, k == 0 ? a.sizes + (size_t)src * (size_t)S : nullptr, tid, SPLIT_THREADS);
}

// One body, two kernels: k_sup_match<false> is pf_join_supports' (`keys` unused: its instructions are those of the kernel
// without the flag); k_sup_match<true> keeps key_of as the running minimum - the same integer min through the wave and
// the workgroup - and writes it to `keys` beside delta, which is derived from it.
template <bool ARG>
__global__ __launch_bounds__(MATCH_THREADS) void k_sup_match(Args a, int32_t* keys) {
    extern __shared__ uint64_t tile[];                         // [TILE][W]
    __shared__ int part[MATCH_WAVES][TILE];
    const int N = a.N, S = N - 3, W = words_of(N), tid = (int)threadIdx.x;
    const int t0 = (int)blockIdx.x * TILE, r = (int)blockIdx.y, src = (int)blockIdx.z;
    const int32_t* sizes = a.sizes + (size_t)src * (size_t)S;
    int32_t* delta = a.delta + ((size_t)src * (size_t)a.rc + (size_t)r) * (size_t)S;
    int32_t* arg = ARG ? keys + ((size_t)src * (size_t)a.rc + (size_t)r) * (size_t)S : nullptr;
    if (flagged(a, src, r + 1)) {                              // (uniform)
        if (tid < TILE && t0 + tid < S) {
            delta[t0 + tid] = delta_of(N, sizes[t0 + tid], N);
            if (ARG) arg[t0 + tid] = key_none(N);
        }
        return;
    }
    tile_load(tile, bits_of(a, src, 0), S, W, t0, tid, MATCH_THREADS);
    __syncthreads();
    int best[TILE];
    match_thread<ARG>(tile, bits_of(a, src, r + 1), S, W, N, tid, MATCH_THREADS, best);
#pragma unroll
    for (int k = 0; k < TILE; ++k) {
        int m = best[k];
        for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, 64));
        if ((tid & 63) == 0) part[tid >> 6][k] = m;
    }
    __syncthreads();
    if (tid < TILE && t0 + tid < S) {
        int m = part[0][tid];
        for (int w = 1; w < MATCH_WAVES; ++w) m = min(m, part[w][tid]);
        delta[t0 + tid] = delta_of(ARG ? key_m(m) : m, sizes[t0 + tid], N);
        if (ARG) arg[t0 + tid] = m;
    }
}

// Every thread of a workgroup reads the same key: handed over as a scalar, so the replicate loop's branches are scalar.
struct UniformKeys {
    __device__ int32_t operator()(const int32_t* p) const { return __builtin_amdgcn_readfirstlane(*p); }
};
// (integer sums: any order gives the same result)
struct AtomicAdd {
    __device__ void operator()(int64_t* p, int32_t c) const { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)c); }
};

// grid (reference splits, sources): the workgroup walks the splits t = blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(MOVES_THREADS) void k_sup_moves(Args a, Transfers x, int first) {
    for (int t = (int)blockIdx.x; t < a.N - 3; t += (int)gridDim.x)
        moves_thread(a, x, (int)blockIdx.y, t, first != 0, (int)threadIdx.x, MOVES_THREADS, UniformKeys{}, AtomicAdd{});
}

__global__ __launch_bounds__(SUM_THREADS) void k_sup_sum(Args a, int first) {
    const int t = (int)blockIdx.x * SUM_THREADS + (int)threadIdx.x;
    if (t < a.N - 3) sum_split(a, (int)blockIdx.y, t, first != 0);
}

// The arrays of a chunk of nb sources with rc replicates each inside `base` (nb * state_bytes(N, rc) bytes at least; with
// `x`, pf_join_transfers' keys too: nb * transfer_state_bytes(N, rc))
inline void carve(Args& a, char* base, Transfers* x = nullptr) {
    const size_t S = (size_t)a.N - 3, W = (size_t)words_of(a.N), trees = (size_t)a.nb * (size_t)(a.rc + 1);
    pfspan::Carve c{base};
    c(a.bits, trees * S * W); c(a.row, trees * (size_t)a.N); c(a.sizes, (size_t)a.nb * S); c(a.delta, (size_t)a.nb * (size_t)a.rc * S);
    if (x) c(x->arg, (size_t)a.nb * (size_t)a.rc * S);
}

// Asynchronous on `s`: one chunk (nb <= SUP_MAX_Y sources, rc <= SUP_MAX_Y replicates, N >= 4).  `first`: the chunk
// starts the sums of its sources.  With `x` (pf_join_transfers) the matching keeps its keys and k_sup_moves follows.
inline hipError_t launch_chunk(hipStream_t s, const Args& a, bool first, const Transfers* x = nullptr) {
    const int S = a.N - 3, W = words_of(a.N);
    const dim3 tiles((unsigned)((S + TILE - 1) / TILE), (unsigned)a.rc, (unsigned)a.nb);
    const size_t lds = (size_t)TILE * (size_t)W * sizeof(uint64_t);
    hipLaunchKernelGGL(k_sup_splits, dim3((unsigned)(a.nb * (a.rc + 1))), dim3(SPLIT_THREADS), 0, s, a);
    if (x) hipLaunchKernelGGL(k_sup_match<true>, tiles, dim3(MATCH_THREADS), lds, s, a, x->arg);
    else hipLaunchKernelGGL(k_sup_match<false>, tiles, dim3(MATCH_THREADS), lds, s, a, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_sup_sum, dim3((unsigned)((S + SUM_THREADS - 1) / SUM_THREADS), (unsigned)a.nb), dim3(SUM_THREADS), 0, s, a,
                       first ? 1 : 0);
    if (x) {
        // (the sum over a source's splits is an atomic one: moves starts at zero; workgroups times threads stay below 2^32)
        if (first) {
            const hipError_t e = hipMemsetAsync(x->moves + (size_t)a.b0 * (size_t)a.N, 0, (size_t)a.nb * (size_t)a.N * sizeof(int64_t), s);
            if (e != hipSuccess) return e;
        }
        const int gx = std::min(S, std::max(1, (1 << 23) / a.nb));
        hipLaunchKernelGGL(k_sup_moves, dim3((unsigned)gx, (unsigned)a.nb), dim3(MOVES_THREADS), 0, s, a, *x, first ? 1 : 0);
    }
    return hipGetLastError();
}

}  // namespace pfsup
