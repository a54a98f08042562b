// Distances between the join tables of one source on the device (pf_join_distances, pf_join_distances_device; DESIGN.md
// section 35): shared splits, the Kuhner-Felsenstein branch score and weighted RF of every pair of K trees - bit for bit
// those of treedist.py::join_distances_py.  The bodies are pf_treedist_host.h's, shared with the CPU; this file is the
// launches.  The only atomics are vector atomics on global memory (pfcon's: the hash table's claim and tally, the error
// word); no cooperative launch, no thread waits for another, no copy to the host and no synchronisation between the
// launches; wave64.
//   k_con_splits   pfcon's own kernel on a pfcon::Args whose replicates are the K trees: grid (trees, sources), one
//   k_con_keys     workgroup per tree for the bitset table, sizes, `above` and `leaf_pos`; then one thread per (tree,
//   k_con_count    split) for the key, and one for the exact hash table (atomicCAS claim, W-word comparison, probe bound).
//   k_td_index     one thread per (tree, split): the rank of its slot among the tree's S slots by counting - every lane of
//                  a wave reads the same slot_of[k], a broadcast - and (slot, split) into the tree's index at that rank.
//                  Counting, not an LDS sort: no barrier, no LDS and no size switch at the 128 KB a tree of 16,384 would
//                  need; S reads per thread are what k_con_rank already pays.  Either gives the same bytes.
//   k_td_pairs     one wave per pair i < j over a flat pair index, grid y the source: lane l is accumulator l of both
//                  sums, the partner split by binary search in the other tree's index, phase C from two length rows
//                  through leaf_pos; __shfl_down in the statement's order; lane 0 takes the root and stores (i, j), (j, i).
//   k_td_finish    one thread per cell: the diagonal, the cells of flagged trees; the status from the error word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_consensus.hip.h"
#include "pf_treedist_host.h"

namespace pftd {

constexpr int FLAT_THREADS = 256;
constexpr int PAIR_THREADS = 256, PAIR_WAVES = PAIR_THREADS / 64;
constexpr int TD_MAX_Y = pfcon::CON_MAX_Y;      // sources (grid y) of one launch
static_assert(LANES == 64, "one lane per accumulator: wave64");

__global__ __launch_bounds__(FLAT_THREADS) void k_td_index(Args a) {
    const int64_t e = (int64_t)blockIdx.x * FLAT_THREADS + (int64_t)threadIdx.x;
    if (e < (int64_t)pfcon::entries_of(a.c)) index_entry(a, (int)blockIdx.y, e);
}

__global__ __launch_bounds__(PAIR_THREADS) void k_td_pairs(Args a) {
    const int lane = (int)threadIdx.x & 63, src = (int)blockIdx.y, K = trees_of(a);
    const int64_t p = (int64_t)blockIdx.x * PAIR_WAVES + ((int)threadIdx.x >> 6);
    if (p >= pairs_of(K)) return;                              // (the whole wave)
    int i = 0, j = 0;
    pair_of(p, K, &i, &j);
    if (!pair_runs(a, src, i, j)) return;                      // (the error word and the flags are earlier launches')
    Acc acc = pair_lane(a, src, i, j, lane);
    for (int s = 32; s > 0; s >>= 1) {
        Acc o;
        o.sq = __shfl_down(acc.sq, s, 64); o.ab = __shfl_down(acc.ab, s, 64); o.hits = __shfl_down(acc.hits, s, 64);
        if (lane < s) acc_merge(acc, o);
    }
    if (lane == 0) pair_store(a, src, i, j, acc);
}

__global__ __launch_bounds__(FLAT_THREADS) void k_td_finish(Args a) {
    const int64_t u = (int64_t)blockIdx.x * FLAT_THREADS + (int64_t)threadIdx.x;
    if (u < (int64_t)trees_of(a) * trees_of(a)) finish_cell(a, (int)blockIdx.y, u);
}

// The arrays of a chunk of a.c.nb sources inside `base` (nb * state_bytes(N, K) bytes at least); returns where the 0xff
// bytes start, where the zeros start and where the state ends.
inline pfcon::Fill carve(Args& a, char* base) {
    pfspan::Carve c{base};
    state_arrays(c, a, (size_t)a.c.nb, (size_t)a.c.R, a.c.N, (size_t)a.c.cap);
    return pfcon::Fill{reinterpret_cast<char*>(a.c.slot_of), reinterpret_cast<char*>(a.c.tally), c.at};
}

// Asynchronous on `s`: one chunk (nb <= TD_MAX_Y sources, K <= MAX_K trees, N >= 4), its state carved and its results
// zeroed by the caller.
inline hipError_t launch_chunk(hipStream_t s, const Args& a, const pfcon::Fill& f) {
    const int K = trees_of(a);
    const int64_t E = (int64_t)pfcon::entries_of(a.c);
    const auto blocks = [](int64_t n, int per) { return (unsigned)((n + per - 1) / per); };
    const unsigned nb = (unsigned)a.c.nb;
    hipError_t e = hipMemsetAsync(f.ones, 0xff, (size_t)(f.zeros - f.ones), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(f.zeros, 0, (size_t)(f.end - f.zeros), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(pfcon::k_con_splits, dim3((unsigned)K, nb), dim3(pfcon::SPLIT_THREADS), 0, s, a.c);
    hipLaunchKernelGGL(pfcon::k_con_keys, dim3(blocks(E, pfcon::FLAT_THREADS), nb), dim3(pfcon::FLAT_THREADS), 0, s, a.c);
    hipLaunchKernelGGL(pfcon::k_con_count, dim3(blocks(E, pfcon::FLAT_THREADS), nb), dim3(pfcon::FLAT_THREADS), 0, s, a.c);
    hipLaunchKernelGGL(k_td_index, dim3(blocks(E, FLAT_THREADS), nb), dim3(FLAT_THREADS), 0, s, a);
    if (K > 1) hipLaunchKernelGGL(k_td_pairs, dim3(blocks(pairs_of(K), PAIR_WAVES), nb), dim3(PAIR_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_td_finish, dim3(blocks((int64_t)K * K, FLAT_THREADS), nb), dim3(FLAT_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace pftd
