// Bootstrap replicates over alignment sites (pf_resample_sites_device, pf_bootstrap): k_resample builds replicate
// bytes in HBM from one upload of the source alignments.
//
// The replicate stream (phyloformer_amd/bootstrap.py::resample_sites is its host twin): replicate r of an alignment of
// L sites takes, at output position l, the source site
//
//   mix64(z)  SplitMix64's finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
//             z ^= z >> 31 (mod 2^64)
//   key  = mix64(seed + 0x9E3779B97F4A7C15)
//   site = ((mix64(key ^ ((r << 32) | l)) >> 32) * L) >> 32        (in [0, L) by construction)
//
// It depends on (seed, r, l, L) only: not on the residues, the batch, the chunking or the device.
//
// k_resample: src uint8 [B][N][L] -> dst uint8 [B][R][N][L] for replicates r_begin .. r_begin + R - 1.  One workgroup
// per (tile of RS_TILE output sites, replicate): its threads draw the tile's sites once into LDS, then copy every
// row of every source through them - the draw's two 64-bit multiplies are paid once per (r, l), not per byte.  A
// thread copies runs of 4 consecutive output sites; consecutive threads write consecutive runs of a row, one 32-bit
// store each when rows are 4-byte aligned (L % 4 == 0 and dst aligned), else byte stores.  The sources are read as
// random bytes of a row (a few hundred KB at most, L2-resident).  Not the bound of a bootstrap: the forwards over the
// replicates are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace pfb {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;          // output sites per workgroup (a multiple of 4: runs never straddle tiles)
constexpr int RS_MAX_Y = 65535;        // replicates per launch (grid y)

__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__host__ __device__ inline uint64_t stream_key(uint64_t seed) { return mix64(seed + 0x9E3779B97F4A7C15ull); }

struct ResampleArgs {
    const uint8_t* src;    // [B][N][L]
    uint8_t* dst;          // [B][R][N][L]
    uint64_t key;          // stream_key(seed)
    int B, N, L;
    int r_begin;           // stream index of dst's replicate 0
    int R;                 // replicates in dst
    int r_first;           // dst replicate of this launch's blockIdx.y = 0
    int vec;               // 1: L % 4 == 0 and dst 4-byte aligned (32-bit stores)
};

// grid (ceil(L / RS_TILE), replicates of this launch), block RS_THREADS
__global__ __launch_bounds__(RS_THREADS) void k_resample(ResampleArgs a) {
    __shared__ int site[RS_TILE];
    const int l0 = blockIdx.x * RS_TILE;
    const int nl = min(RS_TILE, a.L - l0);
    const int rl = a.r_first + (int)blockIdx.y;                       // replicate in dst
    const uint64_t hi = (uint64_t)(uint32_t)(a.r_begin + rl) << 32;
    for (int i = threadIdx.x; i < nl; i += RS_THREADS) {
        const uint64_t z = mix64(a.key ^ (hi | (uint32_t)(l0 + i)));
        site[i] = (int)(((z >> 32) * (uint64_t)(uint32_t)a.L) >> 32);
    }
    __syncthreads();
    const int runs = (nl + 3) / 4;
    const size_t rows = (size_t)a.B * a.N, L = (size_t)a.L;
    const size_t items = rows * (size_t)runs;
    for (size_t it = threadIdx.x; it < items; it += RS_THREADS) {
        const size_t row = it / (size_t)runs;                          // b * N + n
        const int k = 4 * (int)(it - row * (size_t)runs);
        const size_t b = row / (size_t)a.N, n = row - b * (size_t)a.N;
        const uint8_t* s = a.src + row * L;
        uint8_t* d = a.dst + ((b * (size_t)a.R + (size_t)rl) * (size_t)a.N + n) * L + (size_t)(l0 + k);
        if (a.vec) {                                                   // nl % 4 == 0: the run is whole
            const uint32_t v = (uint32_t)s[site[k]] | ((uint32_t)s[site[k + 1]] << 8) |
                               ((uint32_t)s[site[k + 2]] << 16) | ((uint32_t)s[site[k + 3]] << 24);
            *reinterpret_cast<uint32_t*>(d) = v;
        } else {
            for (int j = 0; j < 4 && k + j < nl; ++j) d[j] = s[site[k + j]];
        }
    }
}

// Asynchronous on `s`: every replicate of dst, in launches of at most RS_MAX_Y replicates.
inline hipError_t launch_resample(hipStream_t s, const uint8_t* src, int B, int N, int L, int r_begin, int R, uint64_t seed,
                                  uint8_t* dst) {
    ResampleArgs a{src, dst, stream_key(seed), B, N, L, r_begin, R, 0,
                   (L % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) ? 1 : 0};
    const unsigned tiles = (unsigned)((L + RS_TILE - 1) / RS_TILE);
    for (int r0 = 0; r0 < R; r0 += RS_MAX_Y) {
        a.r_first = r0;
        hipLaunchKernelGGL(k_resample, dim3(tiles, (unsigned)std::min(RS_MAX_Y, R - r0)), dim3(RS_THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pfb
