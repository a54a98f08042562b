// Kernels of the GENERIC (float64, any embed_dim / n_heads) path; rationale and layouts: pf_generic.hip.h, the
// host-side sequence: pf_f64_host.hip.h.
#include "pf_generic.hip.h"
#include "pf_f64_common.hip.h"

namespace pfg {
using namespace pf64;

// Stage the 16 tokens tok[0..15] (valid[j] = 0: a zero row) into xs[j][c] (row stride Ep + 1) and apply
// nn.LayerNorm(E) (biased variance, eps inside the sqrt, model.py:64-66) with the TRUE E: channels E..Ep-1 become 0.
// Lane (g = lane >> 4, j = lane & 15) reduces channels g, g + 4, ... of token j; one wave per block.
__device__ void stage_ln(double* xs, const double* x, const size_t* tok, const int* valid, const double* gam,
                         const double* bet, int E, int Ep, int lane) {
    const int XS = Ep + 1, g = lane >> 4, j = lane & 15;
    for (int i = lane; i < 16 * Ep; i += WAVE) {
        const int jj = i / Ep, c = i - jj * Ep;
        xs[jj * XS + c] = valid[jj] ? x[tok[jj] * Ep + c] : 0.0;
    }
    __syncthreads();
    double* row = xs + j * XS;
    double s = 0.0;
    for (int c = g; c < E; c += 4) s += row[c];
    const double mu = ln_mean(s, Over{E});
    double v = 0.0;
    for (int c = g; c < E; c += 4) { const double d = row[c] - mu; v = fma(d, d, v); }
    const double sd = ln_sd(v, Over{E});
    for (int c = g; c < Ep; c += 4) row[c] = c < E ? (row[c] - mu) / sd * gam[c] + bet[c] : 0.0;
    __syncthreads();
}

// One 16 x 16 output tile: acc += A(tile T) . xs, K = Ep (Ep / 4 steps).  `frag` points at the tile's fragments.
__device__ __forceinline__ d4 tile_mfma(const double* frag, const double* xs, int Ep, int lane, d4 acc) {
    const int XS = Ep + 1, kq = lane >> 4, j = lane & 15;
    const double* b = xs + j * XS + kq;
    const double* a = frag + lane;
    const int S = Ep / 4;
    for (int s = 0; s < S; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[(size_t)s * 64], b[4 * s], acc, 0, 0, 0);
    return acc;
}

// ---- embedding + pair expansion (model.py:138-143, 173-175) ------------------------------------
// EP: the channel count at compile time (64: the precise path and a generic (64, 4) handle keep shifts and masks
// instead of divisions), 0 = a.Ep at run time.
template <int EP>
__global__ void __launch_bounds__(256) kg_embed(EmbedArgs a) {
    const int Ep = EP ? EP : a.Ep;
    const size_t total = (size_t)a.B * a.P * a.L * Ep;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t tok = i / Ep;
        const int c = (int)(i - tok * Ep);
        const int l = (int)(tok % a.L);
        const size_t bp = tok / a.L;
        const int p = (int)(bp % a.P), b = (int)(bp / a.P);
        int ri = a.idx[((size_t)b * a.N + a.pi[p]) * a.L + l], rj = a.idx[((size_t)b * a.N + a.pj[p]) * a.L + l];
        if ((ri >= NA || rj >= NA) && a.bad) *a.bad = 1u;          // sticky flag, as k_embed (pf_device.hip.h)
        ri = min(ri, NA - 1); rj = min(rj, NA - 1);
        a.x[i] = a.table[ri * Ep + c] + a.table[rj * Ep + c];
    }
}

// ---- attention statistics over one axis (attention.py:163-190) ------------------------------------
// Block (one wave) = (line, chunk of CHUNK elements), 16 elements at a time.  The q / k tiles of the fused projection
// come first (k' of the 16 elements into LDS, q' to HBM for the apply kernel), then the v tiles, each multiplied by
// its head's k'.  Every tile's 16 element lanes are summed by one fixed butterfly and added to the block's
// accumulator sacc[SR] in tile order; part[line][chunk][SR] = sacc.
__global__ void __launch_bounds__(WAVE) kg_attn_stats(StatsArgs a) {
    extern __shared__ double lds[];
    __shared__ size_t tok[16];
    __shared__ int valid[16];
    const Arch ar = a.ar;
    const int XS = ar.Ep + 1;
    double* xs = lds;
    double* kl = xs + 16 * XS;              // [16][NH] k' of the tile's elements
    double* sacc = kl + 16 * ar.NH;         // [SR]
    const int lane = threadIdx.x, g = lane >> 4, j = lane & 15;
    const int line = blockIdx.x / a.nchunk, ch = blockIdx.x - line * a.nchunk;
    const int nelem = a.col ? a.P : a.L;
    const int S = ar.Ep / 4, TV = ar.Ep / 16, TF = ar.MF / 16;
    for (int i = lane; i < ar.SR; i += WAVE) sacc[i] = 0.0;
    const int e_end = min(nelem, (ch + 1) * CHUNK);
    // weighted forwards, row attention: site e counts wt times (times 1.0 - exactly - everywhere else)
    const float* wrow = (a.wt && !a.col) ? a.wt + (size_t)(line / a.P) * a.L : nullptr;
    for (int e0 = ch * CHUNK; e0 < e_end; e0 += 16) {
        if (lane < 16) {
            const int e = e0 + lane;
            valid[lane] = e < e_end;
            tok[lane] = token_of(a.col, line, e < e_end ? e : e0, a.P, a.L);
        }
        __syncthreads();
        stage_ln(xs, a.x, tok, valid, a.w.g, a.w.b, ar.E, ar.Ep, lane);
        const bool vj = valid[j] != 0;
        const size_t tj = tok[j];
        const double wt = (wrow && vj) ? (double)wrow[e0 + j] : 1.0;
        for (int T = TV; T < TF; ++T) {                 // q and k: rows 0..NH-1 Wq, NH..2NH-1 Wk
            d4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = a.w.bf[16 * T + g + 4 * r];
            acc = tile_mfma(a.w.af + (size_t)T * S * 64, xs, ar.Ep, lane, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = 16 * (T - TV) + g + 4 * r;
                const double val = (vj && qr < 2 * ar.NH) ? elu1(acc[r]) : 0.0;
                const double valw = val * wt;
                if (qr < ar.NH) { if (vj) a.q[tj * ar.NH + qr] = val; }
                else if (qr < 2 * ar.NH) kl[j * ar.NH + qr - ar.NH] = valw;
                const double s = sum16(valw);
                if (j == 0 && qr < 2 * ar.NH) sacc[ar.Ep + qr] += s;
            }
        }
        __syncthreads();
        for (int T = 0; T < TV; ++T) {                  // v, channel 16 T + g + 4 r, weighted by k'[channel / HD]
            d4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = a.w.bf[16 * T + g + 4 * r];
            acc = tile_mfma(a.w.af + (size_t)T * S * 64, xs, ar.Ep, lane, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * T + g + 4 * r;
                const double kh = (vj && c < ar.E) ? kl[j * ar.NH + c / ar.HD] : 0.0;
                const double s = sum16(kh * acc[r]);        // attention.py:187-188
                if (j == 0) sacc[c] += s;
            }
        }
        __syncthreads();
    }
    for (int i = lane; i < ar.SR; i += WAVE) a.part[((size_t)line * a.nchunk + ch) * ar.SR + i] = sacc[i];
}

// part[line][nchunk][SR] -> stats[line][SR], chunks in index order
__global__ void __launch_bounds__(256) kg_stats_fin(const double* part, double* stats, int nlines, int nchunk, int SR) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nlines * SR) return;
    const size_t line = i / SR, j = i - line * SR;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[(line * nchunk + c) * SR + j];
    stats[i] = s;
}

// ---- attention apply (attention.py:183-195) + residual --------------------------------------------
// o[h, d] = q'[h] / (S_q[h] / count) * (S_kv[h, d] / S_k[h]);  x += Wo o + bo  (out projection on the matrix cores).
__global__ void __launch_bounds__(WAVE) kg_attn_apply(ApplyArgs a) {
    extern __shared__ double lds[];
    __shared__ size_t tok[16];
    __shared__ int valid[16];
    const Arch ar = a.ar;
    const int XS = ar.Ep + 1;
    double* ctx = lds;                      // [Ep]  S_kv / S_k
    double* rq = ctx + ar.Ep;               // [NH]  S_q / count
    double* os = rq + ar.NH;                // [16][XS]
    const int lane = threadIdx.x, g = lane >> 4, j = lane & 15;
    const int line = blockIdx.x / a.nchunk, ch = blockIdx.x - line * a.nchunk;
    const int nelem = a.col ? a.P : a.L;
    const int S = ar.Ep / 4, TV = ar.Ep / 16;
    const double* st = a.stats + (size_t)line * ar.SR;
    for (int c = lane; c < ar.Ep; c += WAVE) ctx[c] = c < ar.E ? st[c] / st[ar.Ep + ar.NH + c / ar.HD] : 0.0;
    const double count = (a.wst && !a.col) ? (double)a.wst[(size_t)(line / a.P) * 4] : a.count;
    for (int h = lane; h < ar.NH; h += WAVE) rq[h] = st[ar.Ep + h] / count;
    const int e_end = min(nelem, (ch + 1) * CHUNK);
    for (int e0 = ch * CHUNK; e0 < e_end; e0 += 16) {
        if (lane < 16) {
            const int e = e0 + lane;
            valid[lane] = e < e_end;
            tok[lane] = token_of(a.col, line, e < e_end ? e : e0, a.P, a.L);
        }
        __syncthreads();
        for (int i = lane; i < 16 * ar.Ep; i += WAVE) {
            const int jj = i / ar.Ep, c = i - jj * ar.Ep;
            double o = 0.0;
            if (valid[jj] && c < ar.E) {
                const int h = c / ar.HD;
                o = a.q[tok[jj] * ar.NH + h] / rq[h] * ctx[c];
            }
            os[jj * XS + c] = o;
        }
        __syncthreads();
        const bool vj = valid[j] != 0;
        double* xt = a.x + tok[j] * ar.Ep;
        for (int T = 0; T < TV; ++T) {
            d4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = a.w.bo[16 * T + g + 4 * r];
            acc = tile_mfma(a.w.ao + (size_t)T * S * 64, os, ar.Ep, lane, acc);
            if (vj) {
#pragma unroll
                for (int r = 0; r < 4; ++r) xt[16 * T + g + 4 * r] += acc[r];
            }
        }
        __syncthreads();
    }
}

// ---- feed-forward (model.py:69-85, 101-104): x += W2 gelu_erf(W1 LN(x) + b1) + b2 -----------------------
// One wave = 16 consecutive tokens.  Hidden tile T (16 units): D of layer 1 in registers, GELU, then its four
// registers are the K steps of layer 2 into the output tiles, accumulated in LDS (ys[j][c]).
__global__ void __launch_bounds__(WAVE) kg_ffn(FfnArgs a) {
    extern __shared__ double lds[];
    __shared__ size_t tok[16];
    __shared__ int valid[16];
    const Arch ar = a.ar;
    const int XS = ar.Ep + 1;
    double* xs = lds;
    double* ys = xs + 16 * XS;
    const int lane = threadIdx.x, g = lane >> 4, j = lane & 15;
    const size_t t0 = (size_t)blockIdx.x * 16;
    if (lane < 16) {
        valid[lane] = t0 + lane < a.ntok;
        tok[lane] = t0 + lane < a.ntok ? t0 + lane : t0;
    }
    for (int i = lane; i < 16 * ar.Ep; i += WAVE) {
        const int jj = i / ar.Ep, c = i - jj * ar.Ep;
        ys[jj * XS + c] = a.w.b2[c];
    }
    __syncthreads();
    stage_ln(xs, a.x, tok, valid, a.w.g, a.w.b, ar.E, ar.Ep, lane);
    const int S = ar.Ep / 4, TV = ar.Ep / 16, TH = ar.FFp / 16;
    double* yrow = ys + j * XS;
    for (int T = 0; T < TH; ++T) {
        d4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = a.w.b1[16 * T + g + 4 * r];
        h = tile_mfma(a.w.a1 + (size_t)T * S * 64, xs, ar.Ep, lane, h);
        double act[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) act[r] = gelu_f64(h[r]);         // nn.GELU(): erf form
        const double* a2 = a.w.a2 + (size_t)T * TV * 4 * 64 + lane;
        for (int Tc = 0; Tc < TV; ++Tc) {
            d4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = yrow[16 * Tc + g + 4 * r];
#pragma unroll
            for (int r = 0; r < 4; ++r) y = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[(size_t)(Tc * 4 + r) * 64], act[r], y, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) yrow[16 * Tc + g + 4 * r] = y[r];
        }
    }
    __syncthreads();
    for (int i = lane; i < 16 * ar.Ep; i += WAVE) {
        const int jj = i / ar.Ep, c = i - jj * ar.Ep;
        if (valid[jj]) a.x[tok[jj] * ar.Ep + c] += ys[jj * XS + c];
    }
}

// ---- head (model.py:158-164, 182-185): per pair, sum over this rank's sites of softplus(w . x + b) ------
// EP = 0: any a.Ep, a lane's channels by an FMA chain from 0 (the generic path, at Ep = 64 too).  EP = 64: the precise
// path, lane = channel: the lane's term is a plain product, which hipcc contracts into wave_sum's first addition
// (fma(w, x, the partner lane's rounded product)) - other bits than the chain's, and the precise path's since round 5.
template <int EP>
__global__ void __launch_bounds__(256) kg_head(HeadArgs a) {
    const int Ep = EP ? EP : a.Ep;
    const int lane = threadIdx.x & 63, line = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= a.nlines) return;
    const double hb = a.hb[0];
    const float* wrow = a.wt ? a.wt + (size_t)(line / a.P) * a.L : nullptr;     // weighted forwards: site l counts wt times
    double acc = 0.0;
    for (int l = 0; l < a.L; ++l) {
        const double* xt = a.x + ((size_t)line * a.L + l) * Ep;
        double d = EP ? a.hw[lane] * xt[lane] : 0.0;
        for (int c = EP ? EP : lane; c < Ep; c += 64) d = fma(a.hw[c], xt[c], d);
        const double z = wave_sum(d) + hb;
        const double sp = z > 20.0 ? z : log1p(exp(z));           // nn.Softplus(beta = 1, threshold = 20)
        acc += wrow ? sp * (double)wrow[l] : sp;
        if (a.sitemap && lane == 0) a.sitemap[(size_t)line * a.L + l] = (float)sp;   // (outside the accumulation chain)
    }
    if (lane == 0) a.osum[line] = acc;
}
__global__ void __launch_bounds__(256) kg_out(const double* osum, float* out, int n, double l_total, const float* wst, int P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)(osum[i] / (wst ? (double)wst[(size_t)(i / P) * 4] : l_total));   // model.py:185: mean over ALL sites
}
__global__ void __launch_bounds__(256) kg_accumulate(double* dst, const double* src, size_t n) {   // shard emulation
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
__global__ void __launch_bounds__(256) kg_narrow(const double* src, float* dst, size_t ntok, int Ep, int E) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ntok * E) return;
    const size_t t = i / E;
    dst[i] = (float)src[t * Ep + (i - t * E)];
}

size_t stats_lds(const Arch& a) { return (size_t)(16 * (a.Ep + 1) + 16 * a.NH + a.SR) * sizeof(double); }
size_t apply_lds(const Arch& a) { return (size_t)(a.Ep + a.NH + 16 * (a.Ep + 1)) * sizeof(double); }
size_t ffn_lds(const Arch& a) { return (size_t)(2 * 16 * (a.Ep + 1)) * sizeof(double); }

// The attribute is process-wide: it is set to the worst case of the supported set (embed_dim 256, 256 heads), the
// same value for every handle, so handles of different architectures never lower each other's limit.
hipError_t set_lds_limits() {
    const Arch a = make_arch(EMAX, EMAX);
    hipError_t e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&kg_attn_stats), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)stats_lds(a))) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&kg_attn_apply), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)apply_lds(a))) != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&kg_ffn), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)ffn_lds(a));
}

static dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
void launch_embed(hipStream_t s, size_t grid, const EmbedArgs& a) {
    hipLaunchKernelGGL(a.Ep == 64 ? kg_embed<64> : kg_embed<0>, dim3((unsigned)grid), dim3(256), 0, s, a);
}
void launch_attn_stats(hipStream_t s, size_t nblocks, const StatsArgs& a) {
    hipLaunchKernelGGL(kg_attn_stats, dim3((unsigned)nblocks), dim3(WAVE), stats_lds(a.ar), s, a);
}
void launch_stats_fin(hipStream_t s, const double* part, double* stats, int nlines, int nchunk, int SR) {
    hipLaunchKernelGGL(kg_stats_fin, grid_of((size_t)nlines * SR), dim3(256), 0, s, part, stats, nlines, nchunk, SR);
}
void launch_attn_apply(hipStream_t s, size_t nblocks, const ApplyArgs& a) {
    hipLaunchKernelGGL(kg_attn_apply, dim3((unsigned)nblocks), dim3(WAVE), apply_lds(a.ar), s, a);
}
void launch_ffn(hipStream_t s, const FfnArgs& a) {
    hipLaunchKernelGGL(kg_ffn, dim3((unsigned)((a.ntok + 15) / 16)), dim3(WAVE), ffn_lds(a.ar), s, a);
}
void launch_head(hipStream_t s, const HeadArgs& a, bool precise) {
    hipLaunchKernelGGL(precise ? kg_head<64> : kg_head<0>, dim3((unsigned)((a.nlines + 3) / 4)), dim3(256), 0, s, a);
}
void launch_out(hipStream_t s, const double* osum, float* out, int n, double l_total, const float* wst, int P) {
    hipLaunchKernelGGL(kg_out, grid_of((size_t)n), dim3(256), 0, s, osum, out, n, l_total, wst, P);
}
void launch_accumulate(hipStream_t s, double* dst, const double* src, size_t n) { hipLaunchKernelGGL(kg_accumulate, grid_of(n), dim3(256), 0, s, dst, src, n); }
void launch_narrow(hipStream_t s, const double* src, float* dst, size_t ntok, int Ep, int E) {
    hipLaunchKernelGGL(kg_narrow, grid_of(ntok * E), dim3(256), 0, s, src, dst, ntok, Ep, E);
}

}  // namespace pfg
