// Derived alignments as lists of source sites (pf_gather_sites_device, pf_forward_sites, pf_forward_windows):
// k_gather_sites builds them in HBM from one upload of the source alignments.
//
// src uint8 [B][N][L] -> dst uint8 [B][S][N][K]: set s of every source takes K source sites, by one of two maps
//
//   affine   site(s, l) = start[s] + l          start: device int32 [..]      (the windows of a scan)
//   table    site(s, l) = sites[s][l]           sites: device int32 [..][K]   (any indices in [0, L): repeats, any order)
//
// (phyloformer_amd/windows.py::cut_sites is the host twin).  The work split is k_resample's (pf_boot.hip.h): one
// workgroup per (tile of GS_TILE output sites, set); a thread copies runs of 4 consecutive output sites of one row,
// consecutive threads write consecutive runs of a row, one 32-bit store each when rows are 4-byte aligned (K % 4 == 0
// and dst aligned), else byte stores.  Table mode stages the tile's indices in LDS once and reads the source as random
// bytes of a row (L2-resident).  Affine mode needs no LDS: a run's four source bytes are contiguous and are read with
// the widest loads their address allows - one dword, two aligned halfwords, or byte + aligned halfword + byte
// (start[s] and L are arbitrary, so nothing is assumed about the alignment of a row or a window).
//
// The host entry points validate their maps before any device work.  A map that only ever existed on the device
// (pf_gather_sites_device) cannot be: an entry outside [0, L) - or a start outside [0, L - K] - is never dereferenced
// (site 0 is read in its place) and raises the sticky flag `bad`, which the next pf_synchronize / pf_memcpy_d2h
// reports as PF_EINVAL.  Not the bound of a scan: the forwards over the windows are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_bytes.hip.h"

namespace pfs {

constexpr int GS_THREADS = 256;
constexpr int GS_TILE = 1024;          // output sites per workgroup (a multiple of 4: runs never straddle tiles)
constexpr int GS_MAX_Y = 65535;        // sets per launch (grid y)

struct GatherArgs {
    const uint8_t* src;    // [B][N][L]
    uint8_t* dst;          // [B][S][N][K]
    const int32_t* sites;  // table mode: [..][K], row s_begin + s for dst's set s
    const int32_t* start;  // affine mode: [..], entry s_begin + s for dst's set s
    unsigned* bad;         // host-mapped sticky flag: a map entry out of range was seen (may be null)
    int B, N, L, K;
    int s_begin;           // map index of dst's set 0
    int S;                 // sets in dst
    int s_first;           // dst set of this launch's blockIdx.y = 0
    int vec;               // 1: K % 4 == 0 and dst 4-byte aligned (32-bit stores)
};

using pfbytes::load_run4;      // four contiguous source bytes at any address (pf_bytes.hip.h)

// grid (ceil(K / GS_TILE), sets of this launch), block GS_THREADS
template <bool TABLE>
__global__ __launch_bounds__(GS_THREADS) void k_gather_sites(GatherArgs a) {
    __shared__ int site[TABLE ? GS_TILE : 1];
    const int l0 = blockIdx.x * GS_TILE;
    const int nl = min(GS_TILE, a.K - l0);
    const int sl = a.s_first + (int)blockIdx.y;                        // set in dst
    int st = 0;
    if (TABLE) {
        const int32_t* map = a.sites + (size_t)(a.s_begin + sl) * (size_t)a.K + (size_t)l0;
        for (int i = threadIdx.x; i < nl; i += GS_THREADS) {
            int v = map[i];
            if ((unsigned)v >= (unsigned)a.L) {                        // (never taken on a validated table)
                if (a.bad) *a.bad = 1u;
                v = 0;
            }
            site[i] = v;
        }
        __syncthreads();
    } else {
        st = a.start[a.s_begin + sl];
        if (st < 0 || st > a.L - a.K) {                                // (never taken on validated starts)
            if (a.bad && threadIdx.x == 0) *a.bad = 1u;
            st = 0;
        }
    }
    const int runs = (nl + 3) / 4;
    const size_t rows = (size_t)a.B * a.N, L = (size_t)a.L, K = (size_t)a.K;
    const size_t items = rows * (size_t)runs;
    for (size_t it = threadIdx.x; it < items; it += GS_THREADS) {
        const size_t row = it / (size_t)runs;                          // b * N + n
        const int k = 4 * (int)(it - row * (size_t)runs);
        const size_t b = row / (size_t)a.N, n = row - b * (size_t)a.N;
        const uint8_t* s = a.src + row * L;
        uint8_t* d = a.dst + ((b * (size_t)a.S + (size_t)sl) * (size_t)a.N + n) * K + (size_t)(l0 + k);
        const int len = min(4, nl - k);
        uint32_t v;
        if (TABLE) {
            v = 0;
            for (int j = 0; j < len; ++j) v |= (uint32_t)s[site[k + j]] << (8 * j);
        } else {
            const uint8_t* p = s + (size_t)st + (size_t)(l0 + k);
            if (len == 4) {
                v = load_run4(p);
            } else {
                v = 0;
                for (int j = 0; j < len; ++j) v |= (uint32_t)p[j] << (8 * j);
            }
        }
        if (a.vec) {                                                   // nl % 4 == 0: the run is whole
            *reinterpret_cast<uint32_t*>(d) = v;
        } else {
            for (int j = 0; j < len; ++j) d[j] = (uint8_t)(v >> (8 * j));
        }
    }
}

// Asynchronous on `s`: sets s_begin .. s_begin + S - 1 of the map into dst [B][S][N][K], in launches of at most
// GS_MAX_Y sets.  Exactly one of sites / start is given.
inline hipError_t launch_gather(hipStream_t s, const uint8_t* src, int B, int N, int L, const int32_t* sites,
                                const int32_t* start, int s_begin, int S, int K, uint8_t* dst, unsigned* bad) {
    GatherArgs a{src, dst, sites, start, bad, B, N, L, K, s_begin, S, 0,
                 (K % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) ? 1 : 0};
    const unsigned tiles = (unsigned)((K + GS_TILE - 1) / GS_TILE);
    for (int s0 = 0; s0 < S; s0 += GS_MAX_Y) {
        a.s_first = s0;
        const dim3 grid(tiles, (unsigned)std::min(GS_MAX_Y, S - s0));
        if (sites) hipLaunchKernelGGL(k_gather_sites<true>, grid, dim3(GS_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_gather_sites<false>, grid, dim3(GS_THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pfs
