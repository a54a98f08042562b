// Host side of the GENERIC (float64, any embed_dim / n_heads) path - included by pf_lib.hip inside its anonymous
// namespace, after pf_handle, fail / HIPCHK, ProfScope, allreduce() and the precise path's host code.  Kernels and
// the rationale: pf_generic.hip.h.
//
//   kg_embed
//   for k in 0..nb-1:
//       kg_attn_stats(row) -> kg_stats_fin -> [all-reduce srow, double]  -> kg_attn_apply(row)
//       kg_attn_stats(col) -> kg_stats_fin                               -> kg_attn_apply(col)
//       kg_ffn
//   kg_head -> [all-reduce osum, double] -> kg_out
// One stream, n_blocks + 1 collectives in a site-sharded run, the same contract as the precise path: the sequence
// depends on (N, L_total) and the architecture alone.
//
// Which handles run it: every handle whose architecture is not (embed_dim 64, n_heads 4) - there is no other path for
// them - and a (64, 4) handle with option "generic" = 1, whose generic weight image is built on the first such forward
// (a default handle costs nothing on the device until then).

// Supported set of pf_create (the reference's own rule embed_dim % n_heads == 0, attention.py:27-31)
bool generic_arch_ok(const pf_weights_t* w) {
    return w->n_alphabet == NA && w->n_blocks >= 1 && w->n_blocks <= 64 && w->embed_dim >= 1 &&
           w->embed_dim <= pfg::EMAX && w->n_heads >= 1 && w->embed_dim % w->n_heads == 0;
}
bool use_generic(const pf_handle* h) { return h->arch_generic || h->generic; }

// ---- weights widened to double, padded, swizzled into A-fragment order ------------------------------
int prepare_generic_weights(pf_handle* h, const float* blob) {
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
    Blob bl{blob};
    const float* emb_w = bl.take((size_t)E * NA);
    const float* emb_b = bl.take(E);
    const size_t o_table = put((size_t)NA * Ep);
    for (int a = 0; a < NA; ++a)
        for (int c = 0; c < E; ++c) D[o_table + (size_t)a * Ep + c] = std::max((double)emb_w[c * NA + a] + (double)emb_b[c], 0.0);
    struct AO { size_t g, b, af, bf, ao, bo; };
    struct FO { size_t g, b, a1, b1, a2, b2; };
    const int nb = h->n_blocks;
    std::vector<AO> ro(nb), co(nb);
    std::vector<FO> fo(nb);
    auto attn = [&](AO& o) {
        const float *g = bl.take(E), *b = bl.take(E), *wq = bl.take((size_t)H * E), *bq = bl.take(H),
                    *wk = bl.take((size_t)H * E), *bk = bl.take(H), *wv = bl.take((size_t)E * E), *bv = bl.take(E),
                    *wo = bl.take((size_t)E * E), *bo = bl.take(E);
        o.g = padded(g, E, Ep); o.b = padded(b, E, Ep);
        // fused [Wv (rows 0..Ep-1, zero past E); Wq (rows Ep..Ep+H-1); Wk (rows Ep+H..Ep+2H-1)]
        o.af = frags(ar.MF / 16, ar.MF, E, [&](int i, int k) {
            if (i < Ep) return i < E ? (double)wv[(size_t)i * E + k] : 0.0;
            const int r = i - Ep;
            return r < H ? (double)wq[(size_t)r * E + k] : r < 2 * H ? (double)wk[(size_t)(r - H) * E + k] : 0.0;
        });
        o.bf = put(ar.MF);
        for (int c = 0; c < E; ++c) D[o.bf + c] = (double)bv[c];
        for (int r = 0; r < H; ++r) { D[o.bf + Ep + r] = (double)bq[r]; D[o.bf + Ep + H + r] = (double)bk[r]; }
        o.ao = frags(Ep / 16, E, E, [&](int i, int k) { return (double)wo[(size_t)i * E + k]; });
        o.bo = padded(bo, E, Ep);
    };
    for (int k = 0; k < nb; ++k) {
        attn(ro[k]);
        attn(co[k]);
        const float *g = bl.take(E), *b = bl.take(E), *w1 = bl.take((size_t)FF * E), *b1 = bl.take(FF),
                    *w2 = bl.take((size_t)E * FF), *b2 = bl.take(E);
        fo[k].g = padded(g, E, Ep); fo[k].b = padded(b, E, Ep);
        fo[k].a1 = frags(FFp / 16, FF, E, [&](int i, int kk) { return (double)w1[(size_t)i * E + kk]; });
        fo[k].b1 = padded(b1, FF, FFp);
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
        fo[k].b2 = padded(b2, E, Ep);
    }
    const size_t o_hw = padded(bl.take(E), E, Ep), o_hb = padded(bl.take(1), 1, 1);
    HIPCHK(h, pfg::set_lds_limits());
    float* dev = nullptr;
    int rc = upload(h, D, &dev);
    if (rc) return rc;
    const double* base = reinterpret_cast<const double*>(dev);
    GenericWeights& gw = h->gw;
    gw.table = base + o_table;
    for (int k = 0; k < nb; ++k) {
        auto A = [&](const AO& o) { return pfg::AttnW{base + o.g, base + o.b, base + o.af, base + o.bf, base + o.ao, base + o.bo}; };
        gw.row.push_back(A(ro[k]));
        gw.col.push_back(A(co[k]));
        gw.ffn.push_back(pfg::FfnW{base + fo[k].g, base + fo[k].b, base + fo[k].a1, base + fo[k].b1, base + fo[k].a2, base + fo[k].b2});
    }
    gw.hw = base + o_hw; gw.hb = base + o_hb;
    gw.ready = true;
    h->blob_copy.clear();
    h->blob_copy.shrink_to_fit();
    return PF_OK;
}

// a (64, 4) handle forced onto the generic kernels builds their image from its host copy of the blob, once
int ensure_generic_weights(pf_handle* h) {
    if (h->gw.ready) return PF_OK;
    if (h->blob_copy.empty()) return fail(h, PF_ESTATE, "generic weight image unavailable");
    return prepare_generic_weights(h, h->blob_copy.data());
}

// ---- workspace (the float64 paths share h->wsp: a handle runs one of them at a time, on one stream) -------
struct GWorkspace { double *x, *q, *part, *srow, *scol, *osum; };
constexpr int GWS_BUFS = 6;
int gchunks(int n) { return (n + pfg::CHUNK - 1) / pfg::CHUNK; }
size_t generic_bytes(const pfg::Arch& ar, int B, int P, int Lloc, size_t off[GWS_BUFS]) {
    const size_t tok = (size_t)B * P * Lloc;
    const size_t parts = std::max((size_t)B * P * gchunks(Lloc), (size_t)B * Lloc * gchunks(P));
    size_t o = 0;
    off[0] = o; o = align_up(o + tok * ar.Ep * 8, 256);
    off[1] = o; o = align_up(o + tok * ar.NH * 8, 256);
    off[2] = o; o = align_up(o + parts * ar.SR * 8, 256);
    off[3] = o; o = align_up(o + (size_t)B * P * ar.SR * 8, 256);
    off[4] = o; o = align_up(o + (size_t)B * std::max(Lloc, 1) * ar.SR * 8, 256);
    off[5] = o; o = align_up(o + (size_t)B * P * 8, 256);
    return o;
}
void generic_carve(char* ws, const size_t off[GWS_BUFS], GWorkspace* w) {
    w->x = (double*)(ws + off[0]); w->q = (double*)(ws + off[1]); w->part = (double*)(ws + off[2]);
    w->srow = (double*)(ws + off[3]); w->scol = (double*)(ws + off[4]); w->osum = (double*)(ws + off[5]);
}
int ensure_generic_workspace(pf_handle* h, int B, int P, int Lloc, GWorkspace* w) {
    size_t off[GWS_BUFS];
    const size_t need = generic_bytes(h->garch, B, P, Lloc, off);
    if (need > h->wsp_bytes) {
        if (h->wsp) { HIPCHK(h, hipStreamSynchronize(h->stream)); hipFree(h->wsp); h->wsp = nullptr; h->wsp_bytes = 0; }
        if (h->ws_bytes + h->ws2_bytes + need > std::max(need, (size_t)h->ws_limit_bytes)) {
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (h->stream2) HIPCHK(h, hipStreamSynchronize(h->stream2));
            if (h->ws) { hipFree(h->ws); h->ws = nullptr; h->ws_bytes = 0; }
            if (h->ws2) { hipFree(h->ws2); h->ws2 = nullptr; h->ws2_bytes = 0; }
        }
        HIPCHK(h, hipMalloc((void**)&h->wsp, need));
        h->wsp_bytes = need;
    }
    generic_carve(h->wsp, off, w);
    return PF_OK;
}

struct GRun {
    GWorkspace w;
    const uint8_t* d_idx;
    float* d_out;
    int B, N, P, Lloc, L_total;
    size_t ntok() const { return (size_t)B * P * Lloc; }
};

// one launcher call, bracketed for the "generic" profile slot and checked
#define PF_GLAUNCH(h, call)                  \
    do {                                     \
        ProfScope ps_((h), K_GENERIC);       \
        call;                                \
        HIPCHK((h), hipGetLastError());      \
    } while (0)

int g_first(pf_handle* h, const GRun& r) {
    if (!r.ntok()) return PF_OK;
    pfg::EmbedArgs a{r.d_idx, h->pair_i, h->pair_j, h->gw.table, r.w.x, r.B, r.N, r.P, r.Lloc, h->garch.Ep, h->bad_idx_dev};
    const size_t blocks = (r.ntok() * h->garch.Ep + 255) / 256;
    PF_GLAUNCH(h, pfg::launch_embed(h->cur, std::min<size_t>(blocks, 1u << 20), a));
    return PF_OK;
}
// statistics of one axis into `stats` ([lines][SR]); an empty shard contributes zeros
int g_stats(pf_handle* h, const GRun& r, const pfg::AttnW& w, int col, double* stats) {
    const int lines = col ? r.B * r.Lloc : r.B * r.P, nelem = col ? r.P : r.Lloc;
    const int SR = h->garch.SR;
    if (!r.ntok()) {
        if (lines) HIPCHK(h, hipMemsetAsync(stats, 0, (size_t)lines * SR * 8, h->cur));
        return PF_OK;
    }
    const int nch = gchunks(nelem);
    pfg::StatsArgs a{r.w.x, r.w.q, r.w.part, w, h->garch, col, r.P, r.Lloc, nch};
    PF_GLAUNCH(h, pfg::launch_attn_stats(h->cur, (size_t)lines * nch, a));
    PF_GLAUNCH(h, pfg::launch_stats_fin(h->cur, r.w.part, stats, lines, nch, SR));
    return PF_OK;
}
int g_apply(pf_handle* h, const GRun& r, const pfg::AttnW& w, int col, const double* stats) {
    if (!r.ntok()) return PF_OK;
    const int lines = col ? r.B * r.Lloc : r.B * r.P, nelem = col ? r.P : r.Lloc;
    const int nch = gchunks(nelem);
    pfg::ApplyArgs a{r.w.x, r.w.q, stats, w, h->garch, col, r.P, r.Lloc, nch, col ? (double)r.P : (double)r.L_total};
    PF_GLAUNCH(h, pfg::launch_attn_apply(h->cur, (size_t)lines * nch, a));
    return PF_OK;
}
// column attention + FFN of block k: site-local
int g_local(pf_handle* h, const GRun& r, int k) {
    if (!r.ntok()) return PF_OK;
    int rc;
    if ((rc = g_stats(h, r, h->gw.col[k], 1, r.w.scol))) return rc;
    if ((rc = g_apply(h, r, h->gw.col[k], 1, r.w.scol))) return rc;
    pfg::FfnArgs f{r.w.x, h->gw.ffn[k], h->garch, r.ntok()};
    PF_GLAUNCH(h, pfg::launch_ffn(h->cur, f));
    if (h->debug_keep) {
        // taps: the residual stream after every block, narrowed to float, true E channels
        const size_t n = r.ntok() * h->garch.E;
        float* tmp = nullptr;
        HIPCHK(h, hipMalloc((void**)&tmp, n * sizeof(float)));
        pfg::launch_narrow(h->cur, r.w.x, tmp, r.ntok(), h->garch.Ep, h->garch.E);
        rc = save_tap(h, "x" + std::to_string(k + 1), tmp, n);
        hipFree(tmp);
        if (rc) return rc;
    }
    return PF_OK;
}
int g_head(pf_handle* h, const GRun& r) {
    const int lines = r.B * r.P;
    if (!r.ntok()) { HIPCHK(h, hipMemsetAsync(r.w.osum, 0, (size_t)lines * 8, h->cur)); return PF_OK; }
    pfg::HeadArgs a{r.w.x, h->gw.hw, h->gw.hb, r.w.osum, lines, r.Lloc, h->garch.Ep};
    PF_GLAUNCH(h, pfg::launch_head(h->cur, a));
    return PF_OK;
}
int g_out(pf_handle* h, const GRun& r, const double* osum) {
    PF_GLAUNCH(h, pfg::launch_out(h->cur, osum, r.d_out, r.B * r.P, (double)r.L_total));
    return PF_OK;
}

// One chunk of a (possibly site-sharded, possibly empty-shard) forward on the handle's main stream.
int forward_chunk_generic(pf_handle* h, const uint8_t* d_idx, int B, int N, int Lloc, int L_total, float* d_out) {
    const int P = N * (N - 1) / 2;
    int rc = ensure_pairs(h, N);
    if (rc) return rc;
    GRun r{};
    r.d_idx = d_idx; r.d_out = d_out; r.B = B; r.N = N; r.P = P; r.Lloc = Lloc; r.L_total = L_total;
    if ((rc = ensure_generic_workspace(h, B, P, Lloc, &r.w))) return rc;
    const bool reduces = reduces_now(h);
    ForwardScope scope(h, reduces);
    h->cur = h->stream;
    if ((rc = g_first(h, r))) return rc;
    for (int k = 0; k < h->n_blocks; ++k) {
        if ((rc = g_stats(h, r, h->gw.row[k], 0, r.w.srow))) return rc;
        if (reduces && (rc = allreduce(h, r.w.srow, (size_t)B * P * h->garch.SR, NCCL_DOUBLE))) return rc;
        if ((rc = g_apply(h, r, h->gw.row[k], 0, r.w.srow))) return rc;
        if ((rc = g_local(h, r, k))) return rc;
    }
    if ((rc = g_head(h, r))) return rc;
    if (reduces && (rc = allreduce(h, r.w.osum, (size_t)B * P, NCCL_DOUBLE))) return rc;
    return g_out(h, r, r.w.osum);
}

// Alignments per chunk under "ws_limit_mb": every rank derives it from the largest shard (one collective sequence
// per chunk).
int generic_chunk_batch(const pf_handle* h, int B, int P, int Lmax) {
    size_t off[GWS_BUFS];
    const size_t per = generic_bytes(h->garch, 1, P, std::max(Lmax, 1), off);
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (size_t)h->ws_limit_bytes / std::max<size_t>(per, 1)));
}

int forward_device_generic(pf_handle* h, const uint8_t* d_idx, int B, int N, int l_begin, int l_end, int L_total,
                           float* d_out) {
    int rc = ensure_generic_weights(h);
    if (rc) return rc;
    const int Lloc = l_end - l_begin, P = N * (N - 1) / 2;
    const int Lmax = h->world > 1 ? std::max(Lloc, (L_total + h->world - 1) / h->world) : Lloc;
    const int cb = generic_chunk_batch(h, B, P, Lmax);
    for (int b0 = 0; b0 < B; b0 += cb) {
        const int nb = std::min(cb, B - b0);
        rc = forward_chunk_generic(h, d_idx ? d_idx + (size_t)b0 * N * Lloc : nullptr, nb, N, Lloc, L_total,
                                   d_out + (size_t)b0 * P);
        if (rc) return rc;
    }
    return PF_OK;
}

// pf_forward_shards_emulated on the generic path: every emulated rank has its own workspace and runs the kernels a
// real rank runs; the collectives are device-side sums in rank order.
int forward_shards_emulated_generic(pf_handle* h, const uint8_t* idx, int B, int N, int L, int nshards, float* out) {
    int rc = ensure_generic_weights(h);
    if (rc) return rc;
    if ((rc = ensure_pairs(h, N))) return rc;
    const int P = N * (N - 1) / 2, SR = h->garch.SR;
    const int step = (L + nshards - 1) / nshards;
    std::vector<GRun> runs;
    std::vector<void*> allocs;
    auto cleanup = [&]() { hipStreamSynchronize(h->stream); for (void* p : allocs) hipFree(p); };
    auto dmalloc = [&](size_t bytes) { void* p = nullptr; if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return (void*)nullptr; allocs.push_back(p); return p; };
    for (int s = 0; s < nshards; ++s) {
        const int lo = std::min(s * step, L), hi = std::min((s + 1) * step, L);
        if (hi <= lo) continue;
        GRun r{};
        r.B = B; r.N = N; r.P = P; r.Lloc = hi - lo; r.L_total = L;
        size_t off[GWS_BUFS];
        const size_t need = generic_bytes(h->garch, B, P, r.Lloc, off);
        char* ws = (char*)dmalloc(need);
        uint8_t* di = (uint8_t*)dmalloc((size_t)B * N * r.Lloc);
        if (!ws || !di) { cleanup(); return fail(h, PF_ENOMEM, "shard workspace allocation failed"); }
        generic_carve(ws, off, &r.w);
        std::vector<uint8_t> local((size_t)B * N * r.Lloc);
        for (int b = 0; b < B; ++b)
            for (int n = 0; n < N; ++n)
                std::memcpy(&local[((size_t)b * N + n) * r.Lloc], &idx[((size_t)b * N + n) * L + lo], r.Lloc);
        if (hipMemcpy(di, local.data(), local.size(), hipMemcpyHostToDevice) != hipSuccess) { cleanup(); return fail(h, PF_EHIP, "idx upload failed"); }
        r.d_idx = di;
        runs.push_back(r);
    }
    double* total = (double*)dmalloc((size_t)B * P * SR * 8);
    float* dout = (float*)dmalloc((size_t)B * P * sizeof(float));
    if (!total || !dout) { cleanup(); return fail(h, PF_ENOMEM, "shard sum buffer"); }
    const bool keep = h->debug_keep;
    h->debug_keep = false;
    h->cur = h->stream;
    auto sum_all = [&](size_t count, bool is_out) {
        hipMemsetAsync(total, 0, count * 8, h->stream);
        for (auto& r : runs)
            pfg::launch_accumulate(h->stream, total, is_out ? r.w.osum : r.w.srow, count);
    };
    for (auto& r : runs) if ((rc = g_first(h, r))) break;
    for (int k = 0; !rc && k < h->n_blocks; ++k) {
        for (auto& r : runs) if ((rc = g_stats(h, r, h->gw.row[k], 0, r.w.srow))) break;
        if (rc) break;
        sum_all((size_t)B * P * SR, false);
        for (auto& r : runs) {
            if ((rc = g_apply(h, r, h->gw.row[k], 0, total))) break;
            if ((rc = g_local(h, r, k))) break;
        }
    }
    if (!rc) for (auto& r : runs) if ((rc = g_head(h, r))) break;
    if (!rc) {
        sum_all((size_t)B * P, true);
        GRun o = runs.front();
        o.d_out = dout;
        rc = g_out(h, o, total);
    }
    if (!rc && (hipMemcpyAsync(out, dout, (size_t)B * P * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess))
        rc = fail(h, PF_EHIP, "result copy failed");
    h->debug_keep = keep;
    cleanup();
    return rc;
}
