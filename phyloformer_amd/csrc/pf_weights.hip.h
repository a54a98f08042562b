// Site weights on the device (pf_forward_weighted*, pf_forward_sites_weighted, pf_bootstrap_weighted): k_weight_sums
// turns the weight rows w [B][L] of a call into what the forward's kernels read per ALIGNMENT,
//
//   wst[b] = { W, 1 / W, b_scale, a_scale }          (WST floats per alignment)
//
//   W        the alignment's weights added in site order, in float, by ONE thread: the association is the site order,
//            whatever the batch, the chunking or the path.  Every entry point takes W from this kernel (the host only
//            repeats the sum to refuse W == 0 before any device work).  All weights 1 give W = L exactly.
//   1 / W    correctly rounded: what k_outsum multiplies the weighted head sums with (1.0f / L for unit weights)
//   b_scale, a_scale   k_rowfin's fp16 range scaling (pf_device.hip.h, "fp16 operand ranges"): q' / mean_w(q') of a site
//            of positive weight is at most W / w_min, so the rule that reads L_total for unit weights reads
//            W / min{w_l > 0} here - the same powers of two when every weight is 1, and unchanged when all weights of
//            an alignment are scaled by a power of two.
//
// A weight that is negative or not finite, or W == 0, can reach this kernel only through the device entry point (the
// host ones refuse first): it raises the sticky flag `bad`, which the next pf_synchronize / pf_memcpy_d2h reports.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfw {

constexpr int WST = 4;             // floats per alignment in wst
constexpr int WS_THREADS = 64;

__global__ __launch_bounds__(WS_THREADS) void k_weight_sums(const float* w, float* wst, int B, int L, unsigned* bad) {
    const int b = blockIdx.x * WS_THREADS + threadIdx.x;
    if (b >= B) return;
    const float* wb = w + (size_t)b * L;
    float W = 0.f, wmin = 3.402823466e38f;
    bool ok = true;
    for (int l = 0; l < L; ++l) {
        const float v = wb[l];
        ok &= v >= 0.f && v <= 3.402823466e38f;
        W += v;                                        // site order
        if (v > 0.f) wmin = fminf(wmin, v);
    }
    ok &= W > 0.f && W <= 3.402823466e38f;
    if (!ok && bad) *bad = 1u;                         // (never taken on validated weights; plain store, any writer wins)
    const float range = __fdiv_rn(W, wmin);                     // L for unit weights
    float b_scale = 1.f;
    for (float lim = 16384.f; lim < range && b_scale > 1.f / 256.f; lim *= 2.f) b_scale *= 0.5f;
    float* o = wst + (size_t)b * WST;
    o[0] = W;
    o[1] = __fdiv_rn(1.f, W);
    o[2] = b_scale;
    o[3] = 1.f / b_scale;                              // (a power of two: exact)
}

// asynchronous on `s`
inline hipError_t launch_weight_sums(hipStream_t s, const float* w, float* wst, int B, int L, unsigned* bad) {
    hipLaunchKernelGGL(k_weight_sums, dim3((unsigned)((B + WS_THREADS - 1) / WS_THREADS)), dim3(WS_THREADS), 0, s, w, wst, B, L, bad);
    return hipGetLastError();
}

}  // namespace pfw
