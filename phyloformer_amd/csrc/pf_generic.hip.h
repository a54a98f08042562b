// The GENERIC path: the forward (phyloformer/model.py:166-187) in float64 for any architecture the reference's
// Phyloformer(n_blocks, n_heads, h_dim) accepts with the shipped alphabet: 1 <= embed_dim <= 256, embed_dim % n_heads
// == 0, FFN width 4 * embed_dim.  Channel and head counts are runtime values (Arch); the default kernels
// (pf_device.hip.h) and the float64 "precise" kernels (pf_precise.hip.h) stay specialised to 64 / 4.
//
// Arithmetic: float64 throughout in the reference's own op order (un-collapsed LayerNorm affine, separate q / k / v /
// out projections, erf-GELU), so the distance from the fp32 reference is the reference's own rounding error on every
// shape - no shape routing, no fp16 range guard, no range re-check.  Fixed-order sums, no atomics: an alignment's bits
// do not depend on the batch it travels in.
//
// Padding: channels are padded to Ep = round_up(E, 16), the FFN width to FFp = round_up(4 E, 16), with zero weights,
// gains and biases; LayerNorm statistics use the true E, so padded channels stay exactly 0.
//
// Dense contractions (fused V / q / k projection, out projection, both FFN layers) run on v_mfma_f64_16x16x4_f64.
// One wave = 16 tokens; the activations of its 16 tokens are staged in LDS (xs[j][c], row stride Ep + 1) and read
// as the B operand (K step s: lane (kq = lane >> 4, j = lane & 15) supplies channel 4 s + kq of token j).  Weights are
// pre-swizzled into A-fragment order on the host and streamed through L2:
//   frag[T][s][lane] = W[16 T + (lane & 15)][4 s + (lane >> 4)]                 (zero outside W)
// so the D register r of lane (g, j) is output row 16 T + g + 4 r of token j.  The FFN's second layer takes its K
// steps from the first layer's D registers directly (K step (T, r) = hidden unit 16 T + kq + 4 r):
//   a2[T][Tc][r][lane] = W2[16 Tc + (lane & 15)][16 T + (lane >> 4) + 4 r]
// and the hidden layer never leaves the registers of its 16 x 16 tile.
//
// Statistics per line (row attention: the sites of a pair; column attention: the pairs of a site): SR = Ep + 2 NH
// doubles, S_kv[Ep] | S_q[NH] | S_k[NH]; each head's q and k are 1-wide (attention.py:155).
// Layout: x [B][P][Lloc][Ep] double, token-major.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfg {

constexpr int NA = 22;
constexpr int EMAX = 256;
constexpr int WAVE = 64;           // one wave per block: 16 tokens per tile
constexpr int CHUNK = 64;          // elements of the reduce axis per statistics / apply block (four 16-element tiles)

struct Arch {
    int E, NH, HD, Ep, FFp, MF, SR;      // MF = Ep + round_up(2 NH, 16): rows of the fused [Wv; Wq; Wk] projection
};
inline Arch make_arch(int E, int NH) {
    Arch a;
    a.E = E; a.NH = NH; a.HD = E / NH;
    a.Ep = (E + 15) / 16 * 16;
    a.FFp = (4 * E + 15) / 16 * 16;
    a.MF = a.Ep + (2 * NH + 15) / 16 * 16;
    a.SR = a.Ep + 2 * NH;
    return a;
}

// weights of one attention sub-block (device, double)
struct AttnW {
    const double *g, *b;       // LayerNorm affine [Ep] (zero past E)
    const double* af;          // [MF / 16][Ep / 4][64] A fragments of [Wv (rows 0..Ep-1); Wq; Wk]
    const double* bf;          // [MF] biases in the same row order
    const double* ao;          // [Ep / 16][Ep / 4][64] A fragments of Wo
    const double* bo;          // [Ep]
};
struct FfnW {
    const double *g, *b;       // [Ep]
    const double* a1;          // [FFp / 16][Ep / 4][64] A fragments of W1
    const double* b1;          // [FFp]
    const double* a2;          // [FFp / 16][Ep / 16][4][64] A fragments of W2 (K steps from layer 1's D registers)
    const double* b2;          // [Ep]
};

struct EmbedArgs {
    const uint8_t* idx; const int16_t *pi, *pj; const double* table; double* x;
    int B, N, P, L, Ep; unsigned* bad;
};
struct StatsArgs {
    const double* x; double* q; double* part; AttnW w; Arch ar;
    int col;            // 0: line = (b, p), elements = sites;  1: line = (b, l), elements = pairs
    int P, L, nchunk;
    const float* wt;    // site weights [B][L] of a weighted forward, or null: a site's
                        // contribution to the ROW statistics counts wt times (the column reductions run over pairs)
};
struct ApplyArgs {
    double* x; const double* q; const double* stats; AttnW w; Arch ar;
    int col, P, L, nchunk;
    double count;       // L_total (row attention) or P (column attention): q / q.mean(dim = -2)
    const float* wst;   // weighted forwards (else null): [B][4], W of the line's alignment at [0] stands for L_total
                        // in the row attention
};
struct FfnArgs { double* x; FfnW w; Arch ar; size_t ntok; };
// sitemap (nullable): float [nlines][L], the softplus term of every token narrowed to float (pf_forward_site_map)
// wt (nullable): site weights float [B][L] of a weighted forward, P pairs per alignment: a site's term counts wt times
struct HeadArgs { const double* x; const double* hw; const double* hb; double* osum; int nlines, L, Ep; float* sitemap;
                  const float* wt; int P; };

// dynamic LDS of the three MFMA kernels for an architecture (bytes)
size_t stats_lds(const Arch& a);
size_t apply_lds(const Arch& a);
size_t ffn_lds(const Arch& a);
// raise the kernels' dynamic-LDS limit to the supported set's worst case (before the first launch)
hipError_t set_lds_limits();

// Launchers (own translation unit: see phyloformer_amd/build.py).  Asynchronous on `s`.  launch_embed, launch_head,
// launch_stats_fin, launch_out, launch_accumulate and launch_narrow serve both float64 paths (the precise one with
// SR = 72, Ep = E = 64).
void launch_embed(hipStream_t s, size_t grid, const EmbedArgs& a);
void launch_attn_stats(hipStream_t s, size_t nblocks, const StatsArgs& a);
void launch_stats_fin(hipStream_t s, const double* part, double* stats, int nlines, int nchunk, int SR);
void launch_attn_apply(hipStream_t s, size_t nblocks, const ApplyArgs& a);
void launch_ffn(hipStream_t s, const FfnArgs& a);
void launch_head(hipStream_t s, const HeadArgs& a, bool precise);     // precise: kg_head<64>, the precise path's bits (Ep = 64)
// wst (nullable; P pairs per alignment): [B][4] of a weighted forward, W at [0] stands for l_total
void launch_out(hipStream_t s, const double* osum, float* out, int n, double l_total, const float* wst = nullptr, int P = 1);
void launch_accumulate(hipStream_t s, double* dst, const double* src, size_t n);
// debug taps: [ntok][Ep] double -> [ntok][E] float
void launch_narrow(hipStream_t s, const double* src, float* dst, size_t ntok, int Ep, int E);

}  // namespace pfg
