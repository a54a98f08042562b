// Host side of the two float64 paths, PRECISE (embed_dim 64, 4 heads: pf_precise.hip.h) and GENERIC (any embed_dim /
// n_heads: pf_generic.hip.h) - included by pf_lib.hip inside its anonymous namespace, after pf_handle, fail / HIPCHK,
// ProfScope, allreduce() and ShardStage.  Both run one schedule, defined once below:
//
//   embed
//   for k in 0..nb-1:
//       attn_stats(row) -> stats_fin -> [all-reduce srow, double]  -> attn_apply(row)
//       attn_stats(col) -> stats_fin                               -> attn_apply(col)
//       ffn
//   head -> [all-reduce osum, double] -> out
// One stream, n_blocks + 1 collectives in a site-sharded run (never cut into halves: every rank selects the path from
// (N, L_total) and the architecture alone, so all ranks issue the same sequence).  The two paths differ only in the
// leaves (F64Path): the launches of attention statistics, apply and FFN with their own kernels; embed, head and the
// tail kernels (stats_fin, out, accumulate, narrow) are pfg's for both.

// Which alignments take the float64 path: a function of the alignment's global shape only (never of the batch).
//   L_total < PRECISE_MAX_SITES : rows shorter than one 32-site tile of k_main.  The distance is a MEAN over sites, and
//                                 on a handful of sites the forward is ill-conditioned in fp32 itself: the fp32 reference
//                                 is 3e-5 ... 8e-4 from its own float64 evaluation there (distances of 20-50), and no
//                                 fp32-level implementation can promise to sit within 1e-4 of ANOTHER fp32-level
//                                 implementation - both are a rounding cloud around the exact value.  float64 sits at the
//                                 cloud's centre: its distance from the reference is the reference's own error.
// Round 6 (fp16 operand split): the default kernels now round at fp32's own level (their distance from float64 equals
// the fp32 reference's, profiles/r06_precise_sweep.txt), so the rule shrank from "< 64 sites, <= 4 sequences or
// < 8,192 tokens" to "< 32 sites or < 8,192 tokens" (round 5: the split-bf16 products' 2^-17 per operand did not average out on small alignments) to rows
// shorter than a tile: with the float64 path off, the sweep's 2,115 cases leave 24 over max(1e-4, 2 x the fp32
// reference's own error), all with <= 24 sites (round 5: 300+, up to 200 sites).
//   P * L_total < PRECISE_MAX_TOKENS : kept from round 5 for tiny alignments of any proportion.  Where the reference's
//                                 own error is near 5e-5 an fp32-level result is over "2 x the reference's own error" by
//                                 chance now and then (one 5 x 33 alignment of random residues in 2,880 soak cases of
//                                 other seeds under the site rule alone: 1.13e-4 against 1.01e-4,
//                                 profiles/r06g_soak_seeds.txt); below 8,192 tokens float64 costs < 0.2 ms.
constexpr int PRECISE_MAX_SITES = 32;
constexpr long PRECISE_MAX_TOKENS = 8192;
bool use_precise(const pf_handle* h, int N, int L_total) {
    // above the option: an alignment / checkpoint whose operands could overflow fp16 never reaches the default kernels
    if (!f16_range_ok(h, N, L_total)) return true;
    if (h->precise >= 0) return h->precise != 0;
    const long P = (long)N * (N - 1) / 2;
    return L_total < PRECISE_MAX_SITES || P * L_total < PRECISE_MAX_TOKENS;
}

// The generic path runs every handle whose architecture is not (embed_dim 64, n_heads 4) - there is no other path for
// them - and a (64, 4) handle with option "generic" = 1, whose generic weight image is built on the first such forward
// (a default handle costs nothing on the device until then).  Its supported set is that of pf_create (the reference's
// own rule embed_dim % n_heads == 0, attention.py:27-31).
bool generic_arch_ok(const pf_weights_t* w) {
    return w->n_alphabet == NA && w->n_blocks >= 1 && w->n_blocks <= 64 && w->embed_dim >= 1 &&
           w->embed_dim <= pfg::EMAX && w->n_heads >= 1 && w->embed_dim % w->n_heads == 0;
}
bool use_generic(const pf_handle* h) { return h->arch_generic || h->generic; }

// ---- precise weights: widened to double, transposed for lane = channel access ---------------------------

int prepare_precise_weights(pf_handle* h, const BlobView& view, PreciseWeights* out) {
    std::vector<double> D;
    auto put = [&D](size_t n) { const size_t o = D.size(); D.resize(o + n); return o; };
    auto copy = [&](const float* src, size_t n) { const size_t o = put(n); for (size_t i = 0; i < n; ++i) D[o + i] = (double)src[i]; return o; };
    auto transposed = [&](const float* src, int M, int K) {          // src[M][K] -> [K][M]
        const size_t o = put((size_t)M * K);
        for (int m = 0; m < M; ++m) for (int k = 0; k < K; ++k) D[o + (size_t)k * M + m] = (double)src[(size_t)m * K + k];
        return o;
    };
    const size_t o_table = put((size_t)NA * E);
    build_embed_table(view, E, E, &D[o_table]);
    struct AO { size_t g, b, wqk, bqk, wvT, bv, woT, bo, a72; };
    struct FO { size_t g, b, w1T, b1, w2T, b2, a1, a2; };
    const int nb = (int)view.ffn.size();
    std::vector<AO> ro(nb), co(nb);
    std::vector<FO> fo(nb);
    auto attn = [&](const AttnHost& a, AO& o) {
        o.g = copy(a.g, E); o.b = copy(a.b, E);
        o.wqk = copy(a.wq, (size_t)NH * E); copy(a.wk, (size_t)NH * E);      // rows 0..3 Wq, 4..7 Wk, contiguous
        o.bqk = copy(a.bq, NH); copy(a.bk, NH);
        o.wvT = transposed(a.wv, E, E); o.bv = copy(a.bv, E);
        o.woT = transposed(a.wo, E, E); o.bo = copy(a.bo, E);
        // A fragments of the fused [Wv; Wq; Wk] projection (pf_precise.hip.h::AttnW)
        o.a72 = put((size_t)5 * 16 * 64);
        for (int T = 0; T < 5; ++T)
            for (int s = 0; s < 16; ++s)
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = lane & 15, c = 16 * (lane >> 4) + s;
                    double v = 0.0;
                    if (T < 4) v = (double)a.wv[(size_t)(16 * T + i) * E + c];
                    else if (i < 4) v = (double)a.wq[(size_t)i * E + c];
                    else if (i < 8) v = (double)a.wk[(size_t)(i - 4) * E + c];
                    D[o.a72 + ((size_t)T * 16 + s) * 64 + lane] = v;
                }
    };
    for (int k = 0; k < nb; ++k) {
        attn(view.row[k], ro[k]);
        attn(view.col[k], co[k]);
        const FfnHost& f = view.ffn[k];
        const float *w1 = f.w1, *w2 = f.w2;
        fo[k].g = copy(f.g, E); fo[k].b = copy(f.b, E);
        fo[k].w1T = transposed(w1, FF, E); fo[k].b1 = copy(f.b1, FF);
        fo[k].w2T = transposed(w2, E, FF); fo[k].b2 = copy(f.b2, E);
        // v_mfma_f64_16x16x4_f64 A fragments of kp_ffn_mfma (layouts: pf_precise.hip.h::FfnW)
        fo[k].a1 = put((size_t)16 * 16 * 64);
        for (int T = 0; T < 16; ++T)
            for (int s = 0; s < 16; ++s)
                for (int lane = 0; lane < 64; ++lane)
                    D[fo[k].a1 + ((size_t)T * 16 + s) * 64 + lane] = (double)w1[(size_t)(16 * T + (lane & 15)) * E + 16 * (lane >> 4) + s];
        fo[k].a2 = put((size_t)16 * 4 * 4 * 64);
        for (int T = 0; T < 16; ++T)
            for (int r = 0; r < 4; ++r)
                for (int tc = 0; tc < 4; ++tc)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 15, kq = lane >> 4;
                        D[fo[k].a2 + (((size_t)T * 4 + r) * 4 + tc) * 64 + lane] =
                            (double)w2[(size_t)(16 * (i & 3) + 4 * tc + (i >> 2)) * FF + 16 * T + kq + 4 * r];
                    }
    }
    const size_t o_hw = copy(view.head_w, E), o_hb = copy(view.head_b, 1);
    float* dev = nullptr;
    int rc = upload(h, D, &dev);
    if (rc) return rc;
    const double* base = reinterpret_cast<const double*>(dev);
    out->blob = reinterpret_cast<double*>(dev);
    out->ends = {base + o_table, base + o_hw, base + o_hb};
    auto A = [&](const AO& o) { return pfp::AttnW{base + o.g, base + o.b, base + o.wqk, base + o.bqk, base + o.wvT, base + o.bv, base + o.woT, base + o.bo, base + o.a72}; };
    for (int k = 0; k < nb; ++k) {
        out->row.push_back(A(ro[k]));
        out->col.push_back(A(co[k]));
        out->ffn.push_back(pfp::FfnW{base + fo[k].g, base + fo[k].b, base + fo[k].w1T, base + fo[k].b1, base + fo[k].w2T, base + fo[k].b2,
                                    base + fo[k].a1, base + fo[k].a2});
    }
    return PF_OK;
}

// ---- generic weights: widened to double, padded, swizzled into A-fragment order -------------------------
int prepare_generic_weights(pf_handle* h, const BlobView& view) {
    const pfg::Arch& ar = h->garch;
    const int E = ar.E, H = ar.NH, Ep = ar.Ep, FF = 4 * E, FFp = ar.FFp, S = Ep / 4;
    std::vector<double> D;
    auto put = [&D](size_t n) { const size_t o = D.size(); D.resize(o + n, 0.0); return o; };
    auto padded = [&](const float* src, int n, int np) { const size_t o = put(np); for (int i = 0; i < n; ++i) D[o + i] = (double)src[i]; return o; };
    // frag[T][s][lane] = W(16 T + (lane & 15), 4 s + (lane >> 4)) for a row-major W[M][K] (zero outside)
    auto frags = [&](int Tn, int M, int K, const std::function<double(int, int)>& W) {
        const size_t o = put((size_t)Tn * S * 64);
        for (int T = 0; T < Tn; ++T)
            for (int s = 0; s < S; ++s)
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = 16 * T + (lane & 15), k = 4 * s + (lane >> 4);
                    if (i < M && k < K) D[o + ((size_t)T * S + s) * 64 + lane] = W(i, k);
                }
        return o;
    };
    const size_t o_table = put((size_t)NA * Ep);
    build_embed_table(view, E, Ep, &D[o_table]);
    struct AO { size_t g, b, af, bf, ao, bo; };
    struct FO { size_t g, b, a1, b1, a2, b2; };
    const int nb = h->n_blocks;
    std::vector<AO> ro(nb), co(nb);
    std::vector<FO> fo(nb);
    auto attn = [&](const AttnHost& a, AO& o) {
        const float *wq = a.wq, *wk = a.wk, *wv = a.wv, *wo = a.wo;
        o.g = padded(a.g, E, Ep); o.b = padded(a.b, E, Ep);
        // fused [Wv (rows 0..Ep-1, zero past E); Wq (rows Ep..Ep+H-1); Wk (rows Ep+H..Ep+2H-1)]
        o.af = frags(ar.MF / 16, ar.MF, E, [&](int i, int k) {
            if (i < Ep) return i < E ? (double)wv[(size_t)i * E + k] : 0.0;
            const int r = i - Ep;
            return r < H ? (double)wq[(size_t)r * E + k] : r < 2 * H ? (double)wk[(size_t)(r - H) * E + k] : 0.0;
        });
        o.bf = put(ar.MF);
        for (int c = 0; c < E; ++c) D[o.bf + c] = (double)a.bv[c];
        for (int r = 0; r < H; ++r) { D[o.bf + Ep + r] = (double)a.bq[r]; D[o.bf + Ep + H + r] = (double)a.bk[r]; }
        o.ao = frags(Ep / 16, E, E, [&](int i, int k) { return (double)wo[(size_t)i * E + k]; });
        o.bo = padded(a.bo, E, Ep);
    };
    for (int k = 0; k < nb; ++k) {
        attn(view.row[k], ro[k]);
        attn(view.col[k], co[k]);
        const FfnHost& f = view.ffn[k];
        const float *w1 = f.w1, *w2 = f.w2;
        fo[k].g = padded(f.g, E, Ep); fo[k].b = padded(f.b, E, Ep);
        fo[k].a1 = frags(FFp / 16, FF, E, [&](int i, int kk) { return (double)w1[(size_t)i * E + kk]; });
        fo[k].b1 = padded(f.b1, FF, FFp);
        // a2[T][Tc][r][lane] = W2[16 Tc + (lane & 15)][16 T + (lane >> 4) + 4 r]
        const int TV = Ep / 16, TH = FFp / 16;
        fo[k].a2 = put((size_t)TH * TV * 4 * 64);
        for (int T = 0; T < TH; ++T)
            for (int Tc = 0; Tc < TV; ++Tc)
                for (int r = 0; r < 4; ++r)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int c = 16 * Tc + (lane & 15), hu = 16 * T + (lane >> 4) + 4 * r;
                        if (c < E && hu < FF)
                            D[fo[k].a2 + (((size_t)T * TV + Tc) * 4 + r) * 64 + lane] = (double)w2[(size_t)c * FF + hu];
                    }
        fo[k].b2 = padded(f.b2, E, Ep);
    }
    const size_t o_hw = padded(view.head_w, E, Ep), o_hb = padded(view.head_b, 1, 1);
    HIPCHK(h, pfg::set_lds_limits());
    float* dev = nullptr;
    int rc = upload(h, D, &dev);
    if (rc) return rc;
    const double* base = reinterpret_cast<const double*>(dev);
    GenericWeights& gw = h->gw;
    gw.ends = {base + o_table, base + o_hw, base + o_hb};
    for (int k = 0; k < nb; ++k) {
        auto A = [&](const AO& o) { return pfg::AttnW{base + o.g, base + o.b, base + o.af, base + o.bf, base + o.ao, base + o.bo}; };
        gw.row.push_back(A(ro[k]));
        gw.col.push_back(A(co[k]));
        gw.ffn.push_back(pfg::FfnW{base + fo[k].g, base + fo[k].b, base + fo[k].a1, base + fo[k].b1, base + fo[k].a2, base + fo[k].b2});
    }
    gw.ready = true;
    h->blob_copy.clear();
    h->blob_copy.shrink_to_fit();
    return PF_OK;
}

// a (64, 4) handle forced onto the generic kernels builds their image from its host copy of the blob, once
int ensure_generic_weights(pf_handle* h) {
    if (h->gw.ready) return PF_OK;
    if (h->blob_copy.empty()) return fail(h, PF_ESTATE, "generic weight image unavailable");
    return prepare_generic_weights(h, read_blob(h->blob_copy.data(), h->n_blocks, h->garch.E, h->garch.NH));
}

// ---- workspace (the float64 paths share h->wsp: a handle runs one of them at a time, on one stream) -------
// C: doubles per token in x, E: true channels among them (taps), NH: heads (q), SR: statistics per line
struct F64Dims { int C, E, NH, SR; };
struct F64Workspace { double *x, *q, *part, *srow, *scol, *osum; };
constexpr int F64_BUFS = 6;
// elements of the reduce axis per apply block, and per statistics block as `part` is sized (the precise MFMA
// statistics kernel's chunks of pfp::CHUNK_MFMA are fewer)
constexpr int F64_CHUNK = 64;
static_assert(pfp::CHUNK == F64_CHUNK && pfg::CHUNK == F64_CHUNK, "float64 chunk sizes");
int f64_chunks(int n) { return (n + F64_CHUNK - 1) / F64_CHUNK; }
size_t f64_bytes(const F64Dims& d, int B, int P, int Lloc, size_t off[F64_BUFS]) {
    const size_t tok = (size_t)B * P * Lloc;
    const size_t parts = std::max((size_t)B * P * f64_chunks(Lloc), (size_t)B * Lloc * f64_chunks(P));
    size_t o = 0;
    off[0] = o; o = align_up(o + tok * d.C * 8, 256);
    off[1] = o; o = align_up(o + tok * d.NH * 8, 256);
    off[2] = o; o = align_up(o + parts * d.SR * 8, 256);
    off[3] = o; o = align_up(o + (size_t)B * P * d.SR * 8, 256);
    off[4] = o; o = align_up(o + (size_t)B * std::max(Lloc, 1) * d.SR * 8, 256);
    off[5] = o; o = align_up(o + (size_t)B * P * 8, 256);
    return o;
}
void f64_carve(char* ws, const size_t off[F64_BUFS], F64Workspace* w) {
    w->x = (double*)(ws + off[0]); w->q = (double*)(ws + off[1]); w->part = (double*)(ws + off[2]);
    w->srow = (double*)(ws + off[3]); w->scol = (double*)(ws + off[4]); w->osum = (double*)(ws + off[5]);
}
int ensure_f64_workspace(pf_handle* h, const F64Dims& d, int B, int P, int Lloc, F64Workspace* w) {
    size_t off[F64_BUFS];
    const size_t need = f64_bytes(d, B, P, Lloc, off);
    if (need > h->wsp.cap) {
        int rc = make_room(h, true, need);              // (releases wsp, so the reserve below only allocates)
        if (rc || (rc = h->wsp.reserve(h, need))) return rc;
    }
    f64_carve(h->wsp, off, w);
    return PF_OK;
}

struct F64Path;
struct F64Run {
    const F64Path* path;
    F64Dims d;
    F64Workspace w;
    const uint8_t* d_idx;
    int B, N, P, Lloc, L_total;
    float* d_smap = nullptr;       // [B][P][Lloc] site map of the head's terms (unsharded site-map calls), or null
    const float* d_w = nullptr;    // weighted forwards (unsharded): site weights [B][Lloc] and what k_weight_sums made
    const float* d_wst = nullptr;  // of them, [B][4] (pf_weights.hip.h); null: an unweighted forward
    size_t ntok() const { return (size_t)B * P * Lloc; }
};

// What differs between the two float64 paths: their weight images and the launches of their own kernels with their
// own argument structs.
// The launches are asynchronous on h->cur; the shared code below brackets and checks them.
struct F64Path {
    int prof;                                       // profile slot: K_PRECISE / K_GENERIC
    F64Dims (*dims)(const pf_handle*);
    int (*prepare)(pf_handle*);                     // the weight image is ready before any forward
    int (*stats_chunk)(const pf_handle*);           // elements of the reduce axis per statistics block
    const F64Ends* (*ends)(const pf_handle*);       // what the shared embed and head kernels read
    void (*stats)(pf_handle*, const F64Run&, int k, int col, size_t grid, int nchunk);
    void (*apply)(pf_handle*, const F64Run&, int k, int col, const double* stats, size_t grid, int nchunk);
    void (*ffn)(pf_handle*, const F64Run&, int k);
};

F64Dims precise_dims(const pf_handle*) { return {pfp::E, pfp::E, pfp::NH, pfp::SROW}; }
int precise_prepare(pf_handle*) { return PF_OK; }
// the VALU statistics kernel (option "precise_ffn_valu") reduces chunks of CHUNK elements, the MFMA one of CHUNK_MFMA
int precise_stats_chunk(const pf_handle* h) { return h->precise_ffn_valu ? pfp::CHUNK : pfp::CHUNK_MFMA; }
const F64Ends* precise_ends(const pf_handle* h) { return &h->pw.ends; }
void precise_stats(pf_handle* h, const F64Run& r, int k, int col, size_t grid, int nchunk) {
    const pfp::AttnW& w = col ? h->pw.col[k] : h->pw.row[k];
    pfp::launch_attn_stats(h->cur, grid, {r.w.x, r.w.q, r.w.part, w, col, r.P, r.Lloc, nchunk, r.d_w}, h->precise_ffn_valu);
}
void precise_apply(pf_handle* h, const F64Run& r, int k, int col, const double* stats, size_t grid, int nchunk) {
    const pfp::AttnW& w = col ? h->pw.col[k] : h->pw.row[k];
    pfp::launch_attn_apply(h->cur, grid, {r.w.x, r.w.q, stats, w, col, r.P, r.Lloc, nchunk, col ? (double)r.P : (double)r.L_total, r.d_wst});
}
void precise_ffn(pf_handle* h, const F64Run& r, int k) {
    pfp::launch_ffn(h->cur, {r.w.x, h->pw.ffn[k], r.ntok()}, h->precise_ffn_valu);
}
const F64Path PRECISE_F64 = {K_PRECISE, precise_dims, precise_prepare, precise_stats_chunk, precise_ends,
                             precise_stats, precise_apply, precise_ffn};

F64Dims generic_dims(const pf_handle* h) { return {h->garch.Ep, h->garch.E, h->garch.NH, h->garch.SR}; }
int generic_stats_chunk(const pf_handle*) { return pfg::CHUNK; }
const F64Ends* generic_ends(const pf_handle* h) { return &h->gw.ends; }
void generic_stats(pf_handle* h, const F64Run& r, int k, int col, size_t grid, int nchunk) {
    const pfg::AttnW& w = col ? h->gw.col[k] : h->gw.row[k];
    pfg::launch_attn_stats(h->cur, grid, {r.w.x, r.w.q, r.w.part, w, h->garch, col, r.P, r.Lloc, nchunk, r.d_w});
}
void generic_apply(pf_handle* h, const F64Run& r, int k, int col, const double* stats, size_t grid, int nchunk) {
    const pfg::AttnW& w = col ? h->gw.col[k] : h->gw.row[k];
    pfg::launch_attn_apply(h->cur, grid, {r.w.x, r.w.q, stats, w, h->garch, col, r.P, r.Lloc, nchunk, col ? (double)r.P : (double)r.L_total, r.d_wst});
}
void generic_ffn(pf_handle* h, const F64Run& r, int k) { pfg::launch_ffn(h->cur, {r.w.x, h->gw.ffn[k], h->garch, r.ntok()}); }
const F64Path GENERIC_F64 = {K_GENERIC, generic_dims, ensure_generic_weights, generic_stats_chunk, generic_ends,
                             generic_stats, generic_apply, generic_ffn};

// The kernels an alignment of (N, L_total) runs on: a float64 path, or nullptr for the default kernels.
const F64Path* f64_path_of(const pf_handle* h, int N, int L_total) {
    if (use_generic(h)) return &GENERIC_F64;
    return use_precise(h, N, L_total) ? &PRECISE_F64 : nullptr;
}

// ---- the schedule, shared by both paths ----------------------------------------------------------------

// one launch, bracketed for the path's profile slot and checked
#define PF_F64LAUNCH(h, r, call)                  \
    do {                                          \
        ProfScope ps_((h), (r).path->prof);       \
        call;                                     \
        HIPCHK((h), hipGetLastError());           \
    } while (0)

int f64_embed(pf_handle* h, const F64Run& r) {
    if (!r.ntok()) return PF_OK;
    const size_t blocks = (r.ntok() * r.d.C + 255) / 256;
    const pfg::EmbedArgs a{r.d_idx, h->pair_i, h->pair_j, r.path->ends(h)->table, r.w.x, r.B, r.N, r.P, r.Lloc, r.d.C,
                           h->bad_idx_dev};
    PF_F64LAUNCH(h, r, pfg::launch_embed(h->cur, std::min<size_t>(blocks, 1u << 20), a));
    return PF_OK;
}
// statistics of one axis into `stats` ([lines][SR]); an empty shard contributes zeros
int f64_stats(pf_handle* h, const F64Run& r, int k, int col, double* stats) {
    const int lines = col ? r.B * r.Lloc : r.B * r.P, nelem = col ? r.P : r.Lloc;
    if (!r.ntok()) {
        if (lines) HIPCHK(h, hipMemsetAsync(stats, 0, (size_t)lines * r.d.SR * 8, h->cur));
        return PF_OK;
    }
    const int chunk = r.path->stats_chunk(h);
    const int nch = (nelem + chunk - 1) / chunk;
    PF_F64LAUNCH(h, r, r.path->stats(h, r, k, col, (size_t)lines * nch, nch));
    PF_F64LAUNCH(h, r, pfg::launch_stats_fin(h->cur, r.w.part, stats, lines, nch, r.d.SR));
    return PF_OK;
}
int f64_apply(pf_handle* h, const F64Run& r, int k, int col, const double* stats) {
    if (!r.ntok()) return PF_OK;
    const int lines = col ? r.B * r.Lloc : r.B * r.P, nch = f64_chunks(col ? r.P : r.Lloc);
    PF_F64LAUNCH(h, r, r.path->apply(h, r, k, col, stats, (size_t)lines * nch, nch));
    return PF_OK;
}
// column attention + FFN of block k: site-local
int f64_local(pf_handle* h, const F64Run& r, int k) {
    if (!r.ntok()) return PF_OK;
    int rc;
    if ((rc = f64_stats(h, r, k, 1, r.w.scol))) return rc;
    if ((rc = f64_apply(h, r, k, 1, r.w.scol))) return rc;
    PF_F64LAUNCH(h, r, r.path->ffn(h, r, k));
    if (h->debug_keep) {
        // taps: the residual stream after every block, narrowed to float, true E channels
        const size_t n = r.ntok() * r.d.E;
        float* tmp = nullptr;
        HIPCHK(h, hipMalloc((void**)&tmp, n * sizeof(float)));
        pfg::launch_narrow(h->cur, r.w.x, tmp, r.ntok(), r.d.C, r.d.E);
        rc = save_tap(h, "x" + std::to_string(k + 1), tmp, n);
        hipFree(tmp);
        if (rc) return rc;
    }
    return PF_OK;
}
int f64_head(pf_handle* h, const F64Run& r) {
    if (!r.ntok()) { HIPCHK(h, hipMemsetAsync(r.w.osum, 0, (size_t)r.B * r.P * 8, h->cur)); return PF_OK; }
    const F64Ends& e = *r.path->ends(h);
    // (the precise path keeps its own instance: its dot product rounds differently from the generic one's at Ep = 64)
    PF_F64LAUNCH(h, r, pfg::launch_head(h->cur, {r.w.x, e.hw, e.hb, r.w.osum, r.B * r.P, r.Lloc, r.d.C, r.d_smap, r.d_w, r.P},
                                        r.path->prof == K_PRECISE));
    return PF_OK;
}
// The schedule, over one rank's run or over every emulated rank's in rank order.  reduce(osum, &sum) stands in for
// the all-reduce of srow (osum false) or of osum and names the buffer every rank reads the sum from.
template <class Reduce>
int f64_schedule(pf_handle* h, F64Run* runs, size_t nruns, Reduce reduce, float* d_out) {
    F64Run* const end = runs + nruns;
    const double* sum = nullptr;
    int rc;
    for (F64Run* r = runs; r != end; ++r) if ((rc = f64_embed(h, *r))) return rc;
    for (int k = 0; k < h->n_blocks; ++k) {
        for (F64Run* r = runs; r != end; ++r) if ((rc = f64_stats(h, *r, k, 0, r->w.srow))) return rc;
        if ((rc = reduce(false, &sum))) return rc;
        for (F64Run* r = runs; r != end; ++r) {
            if ((rc = f64_apply(h, *r, k, 0, sum))) return rc;
            if ((rc = f64_local(h, *r, k))) return rc;
        }
    }
    for (F64Run* r = runs; r != end; ++r) if ((rc = f64_head(h, *r))) return rc;
    if ((rc = reduce(true, &sum))) return rc;
    PF_F64LAUNCH(h, *runs, pfg::launch_out(h->cur, sum, d_out, runs->B * runs->P, (double)runs->L_total, runs->d_wst, runs->P));
    return PF_OK;
}

// One chunk of a (possibly site-sharded, possibly empty-shard) forward on the handle's main stream.
// d_w, d_wst (weighted forwards, unsharded): the chunk's weight rows [B][Lloc] and their sums [B][4].
int forward_chunk_f64(pf_handle* h, const F64Path& path, const uint8_t* d_idx, int B, int N, int Lloc, int L_total,
                      float* d_out, float* d_smap = nullptr, const float* d_w = nullptr, const float* d_wst = nullptr) {
    int rc = ensure_pairs(h, N);
    if (rc) return rc;
    F64Run r{&path, path.dims(h), {}, d_idx, B, N, N * (N - 1) / 2, Lloc, L_total, d_smap, d_w, d_wst};
    if ((rc = ensure_f64_workspace(h, r.d, B, r.P, Lloc, &r.w))) return rc;
    const bool reduces = reduces_now(h);
    ForwardScope scope(h, reduces);
    h->cur = h->stream;
    auto reduce = [&](bool osum, const double** sum) {
        double* buf = osum ? r.w.osum : r.w.srow;
        *sum = buf;
        return reduces ? allreduce(h, buf, (size_t)B * r.P * (osum ? 1 : r.d.SR), NCCL_DOUBLE) : PF_OK;
    };
    return f64_schedule(h, &r, 1, reduce, d_out);
}

// alignments per chunk of a float64 forward of B alignments under "ws_limit_mb" (Lmax: the largest shard's sites)
int f64_chunk_batch(const pf_handle* h, const F64Path& path, int B, int P, int Lmax) {
    size_t off[F64_BUFS];
    const size_t per = f64_bytes(path.dims(h), 1, P, std::max(Lmax, 1), off);
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (size_t)h->ws_limit_bytes / std::max<size_t>(per, 1)));
}

int forward_device_f64(pf_handle* h, const F64Path& path, const uint8_t* d_idx, int B, int N, int l_begin, int l_end,
                       int L_total, float* d_out, const float* d_w = nullptr, const float* d_wst = nullptr) {
    int rc = path.prepare(h);
    if (rc) return rc;
    const int Lloc = l_end - l_begin, P = N * (N - 1) / 2;
    // alignments per chunk under "ws_limit_mb": every rank derives it from the largest shard (one collective
    // sequence per chunk)
    const int Lmax = h->world > 1 ? std::max(Lloc, (L_total + h->world - 1) / h->world) : Lloc;
    const int cb = f64_chunk_batch(h, path, B, P, Lmax);
    for (int b0 = 0; b0 < B; b0 += cb) {
        const int nb = std::min(cb, B - b0);
        rc = forward_chunk_f64(h, path, d_idx ? d_idx + (size_t)b0 * N * Lloc : nullptr, nb, N, Lloc, L_total,
                               d_out + (size_t)b0 * P, nullptr, d_w ? d_w + (size_t)b0 * Lloc : nullptr,
                               d_wst ? d_wst + (size_t)b0 * pfw::WST : nullptr);
        if (rc) return rc;
    }
    return PF_OK;
}

// pf_forward_shards_emulated on a float64 path: every emulated rank has its own workspace and runs the kernels a
// real rank runs; the collectives are device-side sums in rank order.
int forward_shards_emulated_f64(pf_handle* h, const F64Path& path, const uint8_t* idx, int B, int N, int L, int nshards,
                                float* out) {
    int rc = path.prepare(h);
    if (rc) return rc;
    if ((rc = ensure_pairs(h, N))) return rc;
    const int P = N * (N - 1) / 2;
    const F64Dims d = path.dims(h);
    ShardStage stage(h);
    if ((rc = stage.upload(idx, B, N, L, nshards))) return rc;
    std::vector<F64Run> runs;
    for (const ShardStage::Shard& s : stage.shards) {
        F64Run r{&path, d, {}, s.d_idx, B, N, P, s.Lloc, L};
        size_t off[F64_BUFS];
        char* ws = (char*)stage.alloc(f64_bytes(d, B, P, s.Lloc, off));
        if (!ws) return fail(h, PF_ENOMEM, "shard workspace allocation failed");
        f64_carve(ws, off, &r.w);
        runs.push_back(r);
    }
    double* total = (double*)stage.alloc((size_t)B * P * d.SR * 8);
    float* dout = (float*)stage.alloc((size_t)B * P * sizeof(float));
    if (!total || !dout) return fail(h, PF_ENOMEM, "shard sum buffer");
    h->cur = h->stream;
    auto reduce = [&](bool osum, const double** sum) {           // a device-side sum in rank order
        const size_t count = (size_t)B * P * (osum ? 1 : d.SR);
        hipMemsetAsync(total, 0, count * 8, h->stream);
        for (const F64Run& r : runs) pfg::launch_accumulate(h->stream, total, osum ? r.w.osum : r.w.srow, count);
        *sum = total;
        return PF_OK;
    };
    rc = f64_schedule(h, runs.data(), runs.size(), reduce, dout);
    if (!rc && (hipMemcpyAsync(out, dout, (size_t)B * P * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess))
        rc = fail(h, PF_EHIP, "result copy failed");
    return rc;
}
