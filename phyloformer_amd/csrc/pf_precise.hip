// Kernels of the PRECISE (float64) path; rationale, layout and the host-side sequence: pf_precise.hip.h,
// pf_f64_host.hip.h.  Embedding, head and the tail kernels (statistics finish, out, shard sums, taps) are
// pf_generic.hip's.
#include "pf_precise.hip.h"
#include "pf_f64_common.hip.h"

namespace pfp {
using namespace pf64;

// nn.LayerNorm(64), biased variance, eps inside the sqrt (model.py:64-66); lane c holds channel c
__device__ __forceinline__ double layer_norm(double x, double g, double b) {
    const double mu = wave_sum(x) * (1.0 / 64.0);
    const double xc = x - mu;
    const double var = wave_sum(xc * xc) * (1.0 / 64.0);
    return xc / sqrt(var + 1e-5) * g + b;
}

// ---- attention statistics over one axis (attention.py:163-190) ------------------------------------
// Block = (line, chunk of CHUNK elements; lines: pf_f64_common.hip.h::token_of); its four waves take
// the chunk's elements round-robin and leave part[line][chunk][72] = S_kv[64] | S_q[4] | S_k[4] summed in the
// fixed order wave 0 + wave 1 + wave 2 + wave 3.  q' is kept per token for the apply kernel.
__global__ void __launch_bounds__(PT) kp_attn_stats(StatsArgs a) {
    __shared__ double wv[E * E];          // 32 KB: WvT
    __shared__ double red[4][SROW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int line = blockIdx.x / a.nchunk, ch = blockIdx.x - line * a.nchunk;
    const int nelem = a.col ? a.P : a.L;
    for (int i = tid; i < E * E; i += PT) wv[i] = a.w.wvT[i];
    const double g = a.w.g[lane], beta = a.w.b[lane], bv = a.w.bv[lane];
    double wqk[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) wqk[m] = a.w.wqk[m * E + lane];
    const double bqk = a.w.bqk[lane & 7];
    __syncthreads();
    double skv = 0.0, s8 = 0.0;           // lane c: S_kv[c];  lanes 0..7: S_q[0..3], S_k[0..3]
    const int e_end = min(nelem, (ch + 1) * CHUNK);
    // weighted forwards, row attention: site e counts wt times (times 1.0 - exactly - everywhere else)
    const float* wrow = (a.wt && !a.col) ? a.wt + (size_t)(line / a.P) * a.L : nullptr;
    for (int e = ch * CHUNK + w; e < e_end; e += 4) {
        const size_t tok = token_of(a.col, line, e, a.P, a.L);
        const double wt = wrow ? (double)wrow[e] : 1.0;
        const double xn = layer_norm(a.x[tok * E + lane], g, beta);
        double qk = 0.0;                  // lane m < 8 ends up with elu(.)+1 of projection m
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const double s = wave_sum(wqk[m] * xn);
            if ((lane & 7) == m) qk = s;
        }
        qk = elu1(qk + bqk);
        double v = bv;
#pragma unroll 8
        for (int k = 0; k < E; ++k) v = fma(wv[k * E + lane], bcast(xn, k), v);
        const double k0 = bcast(qk, 4), k1 = bcast(qk, 5), k2 = bcast(qk, 6), k3 = bcast(qk, 7);
        const double kh = (lane >> 4) == 0 ? k0 : (lane >> 4) == 1 ? k1 : (lane >> 4) == 2 ? k2 : k3;
        skv += (kh * wt) * v;             // attention.py:187-188: sum of k'[h] * v[h, d], channel h * 16 + d
        if (lane < 8) s8 += qk * wt;
        if (lane < 4) a.q[tok * 4 + lane] = qk;
    }
    red[w][lane] = skv;
    if (lane < 8) red[w][64 + lane] = s8;
    __syncthreads();
    if (tid < SROW) a.part[((size_t)line * a.nchunk + ch) * SROW + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// The same statistics with the projections on the matrix cores (v_mfma_f64_16x16x4_f64; layouts as kp_ffn_mfma below):
// one wave = 16 elements of the line at a time, lane (g, j) holds channels 16 g ... 16 g + 15 of element j.  The fused
// 72 x 64 projection [Wv; Wq; Wk] is five 16-row tiles: tile T < 4 is head T of v (register r of lane (g, j) = channel
// 16 T + g + 4 r), tile 4 leaves q[g] in register 0 and k[g] in register 1 of lane (g, j).  Each lane accumulates the
// contributions of its own elements (k'[T] comes from lane (T, j) by one shuffle); the 16 element lanes of a lane group
// are summed once per wave at the end, the four waves in fixed order.  Block = (line, chunk of CHUNK_MFMA elements).
__global__ void __launch_bounds__(PT) kp_attn_stats_mfma(StatsArgs a) {
    __shared__ double red[4][SROW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, j = lane & 15;
    const int line = blockIdx.x / a.nchunk, ch = blockIdx.x - line * a.nchunk;
    const int nelem = a.col ? a.P : a.L;
    const double* gam = a.w.g + 16 * g;       // (re-read per tile from L1: 64 registers are worth more than 32 loads)
    const double* bet = a.w.b + 16 * g;
    const double bq = a.w.bqk[g], bk = a.w.bqk[4 + g];
    d4 skv[4];
#pragma unroll
    for (int T = 0; T < 4; ++T) skv[T] = d4{0.0, 0.0, 0.0, 0.0};
    double sq = 0.0, sk = 0.0;
    const int e_end = min(nelem, (ch + 1) * CHUNK_MFMA);
    // weighted forwards, row attention: site e counts wt times (times 1.0 - exactly - everywhere else)
    const float* wrow = (a.wt && !a.col) ? a.wt + (size_t)(line / a.P) * a.L : nullptr;
    for (int e0 = ch * CHUNK_MFMA + 16 * w; e0 < e_end; e0 += 64) {
        const int e = e0 + j;
        const bool valid = e < e_end;
        const double wt = (wrow && valid) ? (double)wrow[e] : 1.0;
        const size_t tok = token_of(a.col, line, valid ? e : e0, a.P, a.L);
        double xn[16];
        {
            const double* p = a.x + tok * E + 16 * g;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 16; ++m) { xn[m] = p[m]; s += xn[m]; }
            const double mu = ln_mean(s, Times64th());
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 16; ++m) { xn[m] -= mu; v = fma(xn[m], xn[m], v); }
            const double sd = ln_sd(v, Times64th());
#pragma unroll
            for (int m = 0; m < 16; ++m) xn[m] = xn[m] / sd * gam[m] + bet[m];
        }
        d4 qk = d4{bq, bk, 0.0, 0.0};
        {
            const double* a4 = a.w.a72 + (size_t)4 * 16 * 64 + lane;
#pragma unroll 4
            for (int s = 0; s < 16; ++s) qk = __builtin_amdgcn_mfma_f64_16x16x4f64(a4[s * 64], xn[s], qk, 0, 0, 0);
        }
        const double qp = valid ? elu1(qk[0]) : 0.0, kp = valid ? elu1(qk[1]) : 0.0;     // q'[g], k'[g] of element j
        const double kpw = kp * wt;
        sq += qp * wt;
        sk += kpw;
        if (valid) a.q[tok * 4 + g] = qp;
#pragma unroll
        for (int T = 0; T < 4; ++T) {
            d4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = a.w.bv[16 * T + g + 4 * r];
            const double* aT = a.w.a72 + (size_t)T * 16 * 64 + lane;
#pragma unroll 4
            for (int s = 0; s < 16; ++s) v = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[s * 64], xn[s], v, 0, 0, 0);
            const double kT = __shfl(kpw, 16 * T + j, 64);         // k'[T] of element j (0 for an element past the end)
#pragma unroll
            for (int r = 0; r < 4; ++r) skv[T][r] = fma(kT, v[r], skv[T][r]);   // attention.py:187-188, channel 16 T + g + 4 r
        }
    }
    // sum over the 16 element lanes of each lane group, then over the four waves (fixed order)
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
        for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int r = 0; r < 4; ++r) skv[T][r] += __shfl_xor(skv[T][r], m, 64);
        sq += __shfl_xor(sq, m, 64);
        sk += __shfl_xor(sk, m, 64);
    }
    if (j == 0) {
#pragma unroll
        for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[w][16 * T + g + 4 * r] = skv[T][r];
        red[w][64 + g] = sq;
        red[w][68 + g] = sk;
    }
    __syncthreads();
    if (tid < SROW) a.part[((size_t)line * a.nchunk + ch) * SROW + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---- attention apply (attention.py:183-195) + residual --------------------------------------------
// o[h, d] = q'[h] / (S_q[h] / count) * S_kv[h, d] / S_k[h];  y = Wo o + bo;  x += y.
// The line's mix M[h][c] = sum_d Wo[c][16 h + d] ctx[16 h + d], ctx = S_kv / S_k / (S_q / count), is formed once
// per block; a token then costs four multiply-adds per channel.
__global__ void __launch_bounds__(PT) kp_attn_apply(ApplyArgs a) {
    __shared__ double ctx[E];
    __shared__ double M[NH][E];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int line = blockIdx.x / a.nchunk, ch = blockIdx.x - line * a.nchunk;
    const int nelem = a.col ? a.P : a.L;
    const double* s = a.stats + (size_t)line * SROW;
    const double count = (a.wst && !a.col) ? (double)a.wst[(size_t)(line / a.P) * 4] : a.count;
    if (tid < E) ctx[tid] = s[tid] / s[68 + (tid >> 4)] / (s[64 + (tid >> 4)] / count);
    __syncthreads();
    {
        double m = 0.0;                   // thread (h = w, c = lane)
#pragma unroll
        for (int d = 0; d < 16; ++d) m = fma(a.w.woT[(size_t)(16 * w + d) * E + lane], ctx[16 * w + d], m);
        M[w][lane] = m;
    }
    __syncthreads();
    const double bo = a.w.bo[lane];
    const int e_end = min(nelem, (ch + 1) * CHUNK);
    for (int e = ch * CHUNK + w; e < e_end; e += 4) {
        const size_t tok = token_of(a.col, line, e, a.P, a.L);
        const double* q = a.q + tok * 4;
        double y = bo;
#pragma unroll
        for (int h = 0; h < NH; ++h) y = fma(q[h], M[h][lane], y);
        a.x[tok * E + lane] += y;
    }
}

// ---- feed-forward (model.py:69-85, 101-104): x += W2 gelu_erf(W1 LN(x) + b1) + b2 -----------------------
__global__ void __launch_bounds__(PT) kp_ffn(FfnArgs a) {
    __shared__ double xn[FFN_NT][E];
    __shared__ double hid[FFN_NT][FF];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t t0 = (size_t)blockIdx.x * FFN_NT;
    const double g = a.w.g[lane], beta = a.w.b[lane];
    for (int t = w; t < FFN_NT; t += 4) {
        const size_t tok = t0 + t;
        const double xv = tok < a.ntok ? a.x[tok * E + lane] : 0.0;
        xn[t][lane] = layer_norm(xv, g, beta);
    }
    __syncthreads();
    {
        double acc[FFN_NT];
        const double b1 = a.w.b1[tid];
#pragma unroll
        for (int t = 0; t < FFN_NT; ++t) acc[t] = b1;
        for (int k = 0; k < E; ++k) {
            const double wk = a.w.w1T[(size_t)k * FF + tid];
#pragma unroll
            for (int t = 0; t < FFN_NT; ++t) acc[t] = fma(wk, xn[t][k], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < FFN_NT; ++t) hid[t][tid] = 0.5 * acc[t] * (1.0 + erf(acc[t] * 0.70710678118654752440));   // nn.GELU(): erf form
    }
    __syncthreads();
    {
        // thread (c = lane, token pair w, w + 4)
        double y0 = a.w.b2[lane], y1 = y0;
        for (int j = 0; j < FF; ++j) {
            const double wj = a.w.w2T[(size_t)j * E + lane];
            y0 = fma(wj, hid[w][j], y0);
            y1 = fma(wj, hid[w + 4][j], y1);
        }
        if (t0 + w < a.ntok) a.x[(t0 + w) * E + lane] += y0;
        if (t0 + w + 4 < a.ntok) a.x[(t0 + w + 4) * E + lane] += y1;
    }
}

// ---- the same on the matrix cores: v_mfma_f64_16x16x4_f64 -------------------------------------------------
// One wave = 16 tokens on the N side.  Lane (g = lane >> 4, j = lane & 15) holds the 16 channels 16 g ... 16 g + 15
// of token j - 128 contiguous bytes of x.  Operand layouts (cdna_hip_programming.md): A[i][k] in lane i + 16 k,
// B[k][j] in lane j + 16 k, D[row = g + 4 r][col = j] in register r of lane (g, j).  The K order of each product and
// the row order of each output tile are free, and chosen so that activations never move between lanes:
//   GEMM1  K step s takes channel 16 kq + s from lane group kq            -> B operand = the lane's own xn[s]
//   GEMM1  D tile T: register r of lane (g, j) = hidden unit 16 T + g + 4 r
//   GEMM2  K step (T, r) takes hidden unit 16 T + kq + 4 r from lane group kq  -> B operand = GELU of D register r
//   GEMM2  D tile Tc: row i stands for channel 16 (i & 3) + 4 Tc + (i >> 2), so register r of lane (g, j) is channel
//          16 g + 4 Tc + r: the residual's own layout
// (the A fragments are packed accordingly on the host, pf_f64_host.hip.h).  512 MFMAs per 16 tokens; the
// 256 erf evaluations per token run on the VALU beside another wave's MFMAs.
// (erf-GELU: pf_f64_common.hip.h::gelu_f64)
__global__ void __launch_bounds__(PT) kp_ffn_mfma(FfnArgs a) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const size_t tok = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + j;
    const bool valid = tok < a.ntok;
    double x[16], xn[16];
    {
        const double* p = a.x + (valid ? tok : 0) * E + 16 * g;
#pragma unroll
        for (int m = 0; m < 16; ++m) x[m] = valid ? p[m] : 0.0;
    }
    {   // nn.LayerNorm(64): the token's channels sit in the four lanes (g, j), g = 0..3
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 16; ++m) s += x[m];
        const double mu = ln_mean(s, Times64th());
        double v = 0.0;
#pragma unroll
        for (int m = 0; m < 16; ++m) { xn[m] = x[m] - mu; v = fma(xn[m], xn[m], v); }
        const double sd = ln_sd(v, Times64th());
#pragma unroll
        for (int m = 0; m < 16; ++m) xn[m] = xn[m] / sd * a.w.g[16 * g + m] + a.w.b[16 * g + m];
    }
    d4 y[4];
#pragma unroll
    for (int tc = 0; tc < 4; ++tc)
#pragma unroll
        for (int r = 0; r < 4; ++r) y[tc][r] = a.w.b2[16 * g + 4 * tc + r];
    // The A fragments of one hidden tile T (16 of W1 + 16 of W2 = 16 KB) are the same for the block's four waves: they
    // are staged through LDS, double-buffered - every thread fetches 8 doubles of tile T + 1 while tile T is consumed.
    // (Read straight from L2 by every wave the fragments were 16 KB per TOKEN of L2 traffic: 6.5 TB/s, the kernel's bound.)
    __shared__ double frag[2][2 * 16 * 64];
    const int tid = threadIdx.x;
    {
        const double *s1 = a.w.a1, *s2 = a.w.a2;
#pragma unroll
        for (int k = 0; k < 4; ++k) { frag[0][tid + 256 * k] = s1[tid + 256 * k]; frag[0][1024 + tid + 256 * k] = s2[tid + 256 * k]; }
    }
    __syncthreads();
    for (int T = 0; T < 16; ++T) {
        double n1[4], n2[4];
        const int Tn = min(T + 1, 15);
        {
            const double *s1 = a.w.a1 + (size_t)Tn * 1024, *s2 = a.w.a2 + (size_t)Tn * 1024;
#pragma unroll
            for (int k = 0; k < 4; ++k) { n1[k] = s1[tid + 256 * k]; n2[k] = s2[tid + 256 * k]; }
        }
        const double* f = frag[T & 1];
        d4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = a.w.b1[16 * T + g + 4 * r];
#pragma unroll
        for (int s = 0; s < 16; ++s) h = __builtin_amdgcn_mfma_f64_16x16x4f64(f[s * 64 + lane], xn[s], h, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double act = gelu_f64(h[r]);                                                   // nn.GELU(): erf form
#pragma unroll
            for (int tc = 0; tc < 4; ++tc)
                y[tc] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[1024 + (r * 4 + tc) * 64 + lane], act, y[tc], 0, 0, 0);
        }
        double* fn = frag[(T + 1) & 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) { fn[tid + 256 * k] = n1[k]; fn[1024 + tid + 256 * k] = n2[k]; }
        __syncthreads();
    }
    if (valid) {
        double* p = a.x + tok * E + 16 * g;
#pragma unroll
        for (int tc = 0; tc < 4; ++tc)
#pragma unroll
            for (int r = 0; r < 4; ++r) p[4 * tc + r] = x[4 * tc + r] + y[tc][r];
    }
}

void launch_attn_stats(hipStream_t s, size_t grid, const StatsArgs& a, bool valu) {
    if (valu) hipLaunchKernelGGL(kp_attn_stats, dim3((unsigned)grid), dim3(PT), 0, s, a);
    else hipLaunchKernelGGL(kp_attn_stats_mfma, dim3((unsigned)grid), dim3(PT), 0, s, a);
}
void launch_attn_apply(hipStream_t s, size_t grid, const ApplyArgs& a) { hipLaunchKernelGGL(kp_attn_apply, dim3((unsigned)grid), dim3(PT), 0, s, a); }
void launch_ffn(hipStream_t s, const FfnArgs& a, bool valu) {
    if (valu) hipLaunchKernelGGL(kp_ffn, dim3((unsigned)((a.ntok + FFN_NT - 1) / FFN_NT)), dim3(PT), 0, s, a);
    else hipLaunchKernelGGL(kp_ffn_mfma, dim3((unsigned)((a.ntok + 63) / 64)), dim3(PT), 0, s, a);
}

}  // namespace pfp
