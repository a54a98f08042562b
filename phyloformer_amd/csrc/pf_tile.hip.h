// Tiled inference (pf_forward_tiled, pf_tile_combine_device): the combination of the sets' distances into one matrix.
// The plan - groups, sets, their order - is pf_tile_host.h's; phyloformer_amd/tile.py::combine is the host twin, with
// the same order of additions, and is bit-identical.
//
// sets float [B][T]: the distances of the S = G (G - 1) / 2 sets of every source in (g, h) order, set k at offset[k],
// its m (m - 1) / 2 distances in the reference's pair order among its m = n_g + n_h rows (group g's rows first).
// bounds int32 [G + 1], offset int64 [S + 1]: small device tables built on the host (pftile::Plan).
//
//   out    float [B][P_N]   cross-group pair (i in g, j in h, g < h): its ONE value, in set (g, h), copied bit for bit.
//                           within-group pair of group g: the mean of its G - 1 values, one from every set that contains
//                           g, added in double in ascending order of the partner group, divided by G - 1 and rounded to
//                           float once.
//   spread float [B][P_N]   within-group pair: sqrt( sum (d - mean)^2 / (G - 2) ) over the same G - 1 values in the same
//                           order, in double from the UNROUNDED mean, rounded to float once: the sample standard
//                           deviation of the pair's distance over its contexts.
//                           cross-group pair: exactly 0 - such a pair has one context, so there is no spread to report;
//                           0 here means "not measured", not "certain".
//
// No atomics, no LDS, no cross-lane step: every output element is computed by one thread from (N, M, values) alone, so
// the bits do not depend on B or on the launch.  Floating-point contraction is off in the body: the twin rounds the
// product and the sum of (d - mean)^2 separately.
//   k_tile_combine   one workgroup per output row i (and source), threads striding over j > i.  For a fixed partner
//                    group the reads of a set and the writes of the row are contiguous in j.  All pair indices are
//                    64-bit: P_N exceeds 2^24 at the sizes tiling is for.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pf_taxa_host.h"
#include "pf_tile_host.h"

namespace pftile {

constexpr int TC_THREADS = 256;
constexpr int TC_MAX_Y = 65535;        // sources per launch (grid y)

// grid (N - 1, sources of this launch), block TC_THREADS: row N - 1 has no pair (i, j > i).  The body is
// pftile::combine_row (pf_tile_host.h), which the CPU runs under sanitizers thread by thread.
__global__ __launch_bounds__(TC_THREADS) void k_tile_combine(CombineArgs a) {
    combine_row(a, (int)blockIdx.x, (size_t)blockIdx.y, (int)threadIdx.x, TC_THREADS);
}

// Asynchronous on `s`: sets [B][T] -> out, spread [B][P_N] by the device tables of the plan of (N, G); B >= 1.
inline hipError_t launch_tile_combine(hipStream_t s, const float* sets, const int32_t* bounds, const int64_t* offset, int B, int N,
                                      int G, int64_t T, float* out, float* spread) {
    const int64_t PN = (int64_t)N * (N - 1) / 2;
    for (int b0 = 0; b0 < B; b0 += TC_MAX_Y) {
        const CombineArgs a{sets + (size_t)b0 * (size_t)T, bounds, offset, out + (size_t)b0 * (size_t)PN, spread + (size_t)b0 * (size_t)PN,
                            N, G, T, PN};
        hipLaunchKernelGGL(k_tile_combine, dim3((unsigned)(N - 1), (unsigned)std::min(TC_MAX_Y, B - b0)), dim3(TC_THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pftile
