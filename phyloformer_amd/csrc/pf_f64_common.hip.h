// Device helpers of the two float64 kernel units (pf_precise.hip, pf_generic.hip): each is defined here, once.
#pragma once
#include <hip/hip_runtime.h>

namespace pf64 {

typedef double d4 __attribute__((ext_vector_type(4)));            // C / D of v_mfma_f64_16x16x4_f64

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// sum over the 16 token lanes j of a lane group (fixed butterfly: the same bits on every run)
__device__ __forceinline__ double sum16(double v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double bcast(double v, int lane) {      // `lane` is wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double elu1(double z) { return z > 0.0 ? z + 1.0 : exp(z); }   // attention.py:179-180

// A "line" is what the attention reduces over: the Lloc sites of a pair (row attention, model.py:91) or the P pairs of
// a site (column attention, model.py:97); token_of = the token of element e of a line in x [B][P][L][channels].
__device__ __forceinline__ size_t token_of(int col, int line, int e, int P, int L) {
    if (!col) return (size_t)line * L + e;                       // line = b * P + p, e = l
    const int b = line / L, l = line - b * L;                    // line = b * L + l, e = p
    return ((size_t)b * P + e) * L + l;
}

// nn.LayerNorm statistics (biased variance, eps inside the sqrt, model.py:64-66) of a token whose channels are spread
// over the four lanes (g, j), g = 0..3: `s` / `v` is this lane's partial sum of x / of (x - mu)^2, `over` divides by
// the channel count in the calling kernel's own way (Times64th and Over round differently in general).
struct Times64th { __device__ double operator()(double v) const { return v * (1.0 / 64.0); } };
struct Over { int n; __device__ double operator()(double v) const { return v / (double)n; } };
__device__ __forceinline__ double sum_groups(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
template <class Div> __device__ __forceinline__ double ln_mean(double s, Div over) { return over(sum_groups(s)); }
template <class Div> __device__ __forceinline__ double ln_sd(double v, Div over) { return sqrt(over(sum_groups(v)) + 1e-5); }

// erf-GELU in double without ocml's erf (four divergent ranges, ~2,000 cycles per wave: it was 70 % of the FFN kernel):
//   gelu(h) = max(h, 0) - |h| Q(|h|),  Q(u) = erfc(u / sqrt 2) / 2 = exp(-u^2 / 2) R(u),
//   R(u) (1 + u) = a degree-22 polynomial in t = (u - 4) / (u + 4)  (Chebyshev fit on u in [0, inf), |relative error|
//   of R <= 2.4e-15, coefficients generated with scipy's erfcx; |gelu error| <= 1.8e-15 over |h| <= 40 against
//   0.5 h (1 + erf(h / sqrt 2)) evaluated in double).  Branch-free: one division, one exp, 23 FMAs.
__device__ __forceinline__ double gelu_f64(double h) {
    constexpr double Q[23] = {0x1.e361ea6fba145p-2, -0x1.8c18f2086e47cp-4, 0x1.cabd72a6120b9p-7, 0x1.d4969f10f90d4p-6,
                              -0x1.07c3c25842975p-5, 0x1.25dd720375999p-6, -0x1.47d5fc6944b2cp-8, -0x1.2b7f5644197fap-12,
                              0x1.6c5380196e928p-11, -0x1.8c1283b1235e3p-14, -0x1.707b3dae24d79p-14, 0x1.64919115d4a57p-16,
                              0x1.c9344f4725c3dp-17, -0x1.cdc5363466f39p-19, -0x1.5e69413cc4adcp-19, 0x1.c1cd90ff96cf7p-22,
                              0x1.26fb2b6228421p-21, -0x1.005dbc607bf3dp-26, -0x1.d50a583370aa4p-24, -0x1.1cca57b6a492fp-27,
                              0x1.241e7aeedd9aap-26, 0x1.b830e247ca68bp-30, -0x1.925d735408ab7p-30};
    const double u = fabs(h);
    const double r = 1.0 / ((u + 4.0) * (u + 1.0));
    const double t = (u - 4.0) * (u + 1.0) * r;
    double p = Q[22];
#pragma unroll
    for (int k = 21; k >= 0; --k) p = fma(p, t, Q[k]);
    const double q = exp(-0.5 * u * u) * p * (u + 4.0) * r;
    return fmax(h, 0.0) - u * q;
}

}  // namespace pf64
