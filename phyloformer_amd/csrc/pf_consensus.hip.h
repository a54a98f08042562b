// Majority-rule consensus of replicate join tables on the device (pf_join_consensus, pf_join_consensus_device; DESIGN.md
// section 25): the selected splits of R replicate trees in canonical order, nested into a multifurcating tree, with
// their counts and mean branch lengths - bit for bit those of consensus.py::join_consensus.  The bodies are
// pf_consensus_host.h's, shared with the CPU; this file is the launches.  The only atomics are vector atomics on global
// memory (the hash table's claim and tally, the selection's counter, the error word); no cooperative launch, no thread
// waits for another, no copy to the host and no synchronisation between the launches.
//   k_con_splits   grid (replicates, sources), one workgroup per tree: pfsup's walk of the joins (every thread checks the
//                  join, strides over the words of its row) with, beside it, where the table's lengths hold the branch
//                  above every cluster and leaf; then the normalisation with every split's size.  A table that is no
//                  join table never indexes memory: the walk stops and the source's error word says so.
//   k_con_keys     one thread per (replicate, split): hash and lowest member; lanes read neighbouring words (word-major).
//   k_con_count    one thread per (replicate, split): probes the source's open-addressing table from its hash - at most
//                  `cap` probes, then the error word -, claims an empty slot with atomicCAS, compares an occupied one by
//                  hash and then by all W words, and counts with atomicAdd.
//   k_con_select   one thread per slot: 100 c > F R, compacted in any order.
//   k_con_rank     one thread per selected slot: its rank by (size, lowest member), its words into the rank-ordered table.
//   k_con_nest     grid (tiles of TILE selected splits, sources): the tile's words in LDS; every thread walks the
//                  candidates of larger rank j, loads each word once (neighbouring lanes, neighbouring addresses), tests
//                  child & ~candidate against the whole tile (an LDS broadcast) and keeps the least j; the wave's minimum
//                  by lane shuffles, the workgroup's through LDS.
//   k_con_leaves   one thread per leaf: the least rank that holds it, early exit.
//   k_con_lengths  one thread per (replicate, split): its branch length into lens[rank][r], through slot and rank.
//   k_con_finish   one thread per selected split and per leaf: the sums in ascending replicate order; n_splits, status.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_consensus_host.h"
#include "pf_support.hip.h"

namespace pfcon {

constexpr int SPLIT_THREADS = 256;
constexpr int FLAT_THREADS = 256;       // the kernels of one thread per entry, slot, split or leaf
constexpr int NEST_THREADS = 256, NEST_WAVES = NEST_THREADS / 64;
constexpr int CON_MAX_Y = 65535;        // sources (grid y) of one launch
constexpr int MAX_W = pfsup::MAX_W;     // the tile is TILE * MAX_W * 8 = 32 KB of LDS

struct AtomicTable {
    __device__ int32_t claim(int32_t* owner, int32_t e) const { return atomicCAS(owner, NONE, e); }
    __device__ void add(int32_t* tally) const { atomicAdd(tally, 1); }
    __device__ void raise(int32_t* err, int bits) const { atomicOr(err, bits); }
};

__global__ __launch_bounds__(SPLIT_THREADS) void k_con_splits(Args a) {
    const int N = a.N, S = N - 3, W = words_of(N), tid = (int)threadIdx.x;
    const int r = (int)blockIdx.x, src = (int)blockIdx.y;
    if (flagged(a, src, r)) return;                           // (the whole workgroup)
    const int32_t* slots = slots_of(a, src, r);
    uint64_t* bits = bits_of(a, src, r);
    const size_t k = tree_index(a, src, r);
    int32_t *row = a.row + k * (size_t)N, *above = a.above + k * (size_t)S, *leaf_pos = a.leaf_pos + k * (size_t)N;
    const pfsup::UniformRows rows{row};
    pfsup::rows_init(row, N, tid, SPLIT_THREADS);
    __syncthreads();
    // as k_sup_splits: every thread checks the join itself (the same verdict), thread 0 alone writes `row` - and the
    // branch positions - between two barriers
    bool ok = true;
    for (int t = 0; t < S; ++t) {
        const int32_t sa = slots[2 * t], sb = slots[2 * t + 1];
        int32_t ra = 0, rb = 0;
        if (!pfsup::join_ok(rows, N, sa, sb, &ra, &rb)) { ok = false; break; }
        __syncthreads();
        if (tid == 0) {
            branch_at(above, leaf_pos, sa, ra, 2 * t);
            branch_at(above, leaf_pos, sb, rb, 2 * t + 1);
            row[sa] = t;
            row[sb] = pfsup::DEAD;
        }
        pfsup::join_words(bits, S, W, t, sa, ra, sb, rb, tid, SPLIT_THREADS);
        __syncthreads();
    }
    if (ok) ok = pfsup::final_ok(rows, N, slots + 2 * (size_t)S);
    if (!ok) {
        if (tid == 0) AtomicTable{}.raise(a.err + src, ERR_TABLE);
        return;
    }
    // (three lanes, three slots: read plainly, not through the workgroup-uniform `rows`)
    if (tid < 3) branch_at(above, leaf_pos, slots[2 * S + tid], row[slots[2 * S + tid]], 2 * S + tid);
    pfsup::normalise(bits, S, W, N, a.sizes + k * (size_t)S, tid, SPLIT_THREADS);
}

__global__ __launch_bounds__(FLAT_THREADS) void k_con_keys(Args a) {
    const int64_t e = (int64_t)blockIdx.x * FLAT_THREADS + (int64_t)threadIdx.x;
    if (e < (int64_t)entries_of(a)) keys_entry(a, (int)blockIdx.y, e);
}

__global__ __launch_bounds__(FLAT_THREADS) void k_con_count(Args a) {
    const int64_t e = (int64_t)blockIdx.x * FLAT_THREADS + (int64_t)threadIdx.x;
    if (e < (int64_t)entries_of(a)) count_entry(a, AtomicTable{}, (int)blockIdx.y, e);
}

__global__ __launch_bounds__(FLAT_THREADS) void k_con_select(Args a) {
    const int64_t slot = (int64_t)blockIdx.x * FLAT_THREADS + (int64_t)threadIdx.x;
    const int src = (int)blockIdx.y;
    if (slot < a.cap && select_slot(a, src, slot)) select_put(a, AtomicTable{}, src, slot, atomicAdd(a.nsel + src, 1));
}

__global__ __launch_bounds__(FLAT_THREADS) void k_con_rank(Args a) {
    const int i = (int)blockIdx.x * FLAT_THREADS + (int)threadIdx.x, src = (int)blockIdx.y;
    if (i < selected_count(a, src)) rank_selected(a, AtomicTable{}, src, i);
}

__global__ __launch_bounds__(NEST_THREADS) void k_con_nest(Args a) {
    extern __shared__ uint64_t tile[];                         // [TILE][W]
    __shared__ int part[NEST_WAVES][TILE];
    const int N = a.N, S = N - 3, W = words_of(N), tid = (int)threadIdx.x;
    const int t0 = (int)blockIdx.x * TILE, src = (int)blockIdx.y;
    if (a.err[src]) return;                                    // (uniform: the error word is an earlier launch's)
    const int M = selected_count(a, src);
    if (t0 >= M) return;
    const uint64_t* cbits = cbits_of(a, src);
    tile_load(tile, cbits, S, W, M, t0, tid, NEST_THREADS);
    __syncthreads();
    int best[TILE];
    nest_thread(tile, cbits, S, W, M, t0, tid, NEST_THREADS, best);
#pragma unroll
    for (int k = 0; k < TILE; ++k) {
        int m = best[k];
        for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, 64));
        if ((tid & 63) == 0) part[tid >> 6][k] = m;
    }
    __syncthreads();
    if (tid < TILE && t0 + tid < M) {
        int m = part[0][tid];
        for (int w = 1; w < NEST_WAVES; ++w) m = min(m, part[w][tid]);
        nest_put(a, src, t0 + tid, m);
    }
}

__global__ __launch_bounds__(FLAT_THREADS) void k_con_leaves(Args a) {
    const int x = (int)blockIdx.x * FLAT_THREADS + (int)threadIdx.x, src = (int)blockIdx.y;
    if (x < a.N && !a.err[src]) nest_leaf(a, src, x);
}

__global__ __launch_bounds__(FLAT_THREADS) void k_con_lengths(Args a) {
    const int64_t e = (int64_t)blockIdx.x * FLAT_THREADS + (int64_t)threadIdx.x;
    if (e < (int64_t)entries_of(a)) length_entry(a, (int)blockIdx.y, e);
}

__global__ __launch_bounds__(FLAT_THREADS) void k_con_finish(Args a) {
    const int u = (int)blockIdx.x * FLAT_THREADS + (int)threadIdx.x;
    if (u < a.N - 3 + a.N) finish_thread(a, (int)blockIdx.y, u);
}

// The arrays of a chunk of a.nb sources inside `base` (nb * state_bytes(N, R) bytes at least); returns where the 0xff
// bytes start, where the zeros start and where the state ends.
struct Fill { char *ones, *zeros, *end; };
inline Fill carve(Args& a, char* base) {
    pfspan::Carve c{base};
    state_arrays(c, a, (size_t)a.nb, (size_t)a.R, a.N, (size_t)a.cap, a.rep_lengths != nullptr);
    return Fill{reinterpret_cast<char*>(a.slot_of), reinterpret_cast<char*>(a.tally), c.at};
}

// Asynchronous on `s`: one chunk (nb <= CON_MAX_Y sources, R <= CON_MAX_Y replicates, N >= 4), its state carved and
// its results zeroed by the caller.
inline hipError_t launch_chunk(hipStream_t s, const Args& a, const Fill& f) {
    const int S = a.N - 3, W = words_of(a.N);
    const int64_t E = (int64_t)entries_of(a);
    const auto blocks = [](int64_t n) { return (unsigned)((n + FLAT_THREADS - 1) / FLAT_THREADS); };
    const unsigned nb = (unsigned)a.nb;
    hipError_t e = hipMemsetAsync(f.ones, 0xff, (size_t)(f.zeros - f.ones), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(f.zeros, 0, (size_t)(f.end - f.zeros), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_con_splits, dim3((unsigned)a.R, nb), dim3(SPLIT_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_con_keys, dim3(blocks(E), nb), dim3(FLAT_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_con_count, dim3(blocks(E), nb), dim3(FLAT_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_con_select, dim3(blocks(a.cap), nb), dim3(FLAT_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_con_rank, dim3(blocks(S), nb), dim3(FLAT_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_con_nest, dim3((unsigned)((S + TILE - 1) / TILE), nb), dim3(NEST_THREADS),
                       (size_t)TILE * (size_t)W * sizeof(uint64_t), s, a);
    hipLaunchKernelGGL(k_con_leaves, dim3(blocks(a.N), nb), dim3(FLAT_THREADS), 0, s, a);
    if (a.rep_lengths) hipLaunchKernelGGL(k_con_lengths, dim3(blocks(E), nb), dim3(FLAT_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_con_finish, dim3(blocks(S + a.N), nb), dim3(FLAT_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace pfcon
