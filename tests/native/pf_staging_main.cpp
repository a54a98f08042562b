// Stand-alone check of the staging lists for AddressSanitizer / UBSan builds (tests/test_staging_native.py): what the host
// entry points carve from one grow-only device buffer each, described once per layout and driven by the visitors of
// csrc/pf_spans.h - the staging of pf_nj_joins (pf_nj_host.h) and of pf_join_supports (pf_support_host.h), the two
// tables of the tiling plan (pf_tile_host.h), the float spans of leave-one-out and of placement (pf_lib.hip hands them
// to pfspan::float_spans as they stand here), and the workspace of the attention operator (pfspan::mha_arrays).
//
//     pf_staging_main
//
// For every list and shape: measure it, carve it from a buffer of exactly that many bytes (aligned as a device
// allocation is), record every array behind the carving visitor, and check that
//   - every array is aligned for its element type,
//   - every array lies inside the measured total,
//   - the arrays are pairwise disjoint,
//   - the total is at most 8 bytes per array (256 for the attention operator) above the formula the layout had when
//     it was a chain of byte offsets, and not below it.
// Shapes: N in {3, 4, 9, 65} (supports: N >= 4, a tree of 3 has no split), chunk or B in {1, 3}, R or Q in {1, 3};
// the tiling plans of (N, M) = (5, 2), (9, 4), (65, 16).  The odd counts leave the narrow arrays off alignment.
// Exit code 0 = all hold, 1 = one does not (named on stderr).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_nj_host.h"
#include "../../phyloformer_amd/csrc/pf_support_host.h"
#include "../../phyloformer_amd/csrc/pf_tile_host.h"

namespace {

struct Span { const char* lo; size_t bytes, align_of; };

// carves, and keeps what it handed out
struct Record {
    pfspan::Carve c;
    std::vector<Span> spans;
    template <class T> void operator()(T*& p, size_t count) {
        c(p, count);
        spans.push_back({reinterpret_cast<const char*>(p), count * sizeof(T), alignof(T)});
    }
};

bool ok = true;

// `former`: the bytes of the offset chain
template <class List>
void check(const char* what, int n, int b, int r, List&& list, size_t former, size_t align = 8) {
    const size_t total = pfspan::measure(list, align);
    char* base = static_cast<char*>(aligned_alloc(256, pfspan::up(total, 256)));
    Record rec{{base, align}, {}};
    list(rec);
    auto bad = [&](const char* why, size_t i) {
        fprintf(stderr, "pf_staging_main: %s N=%d B=%d R=%d: array %zu %s\n", what, n, b, r, i, why);
        ok = false;
    };
    for (size_t i = 0; i < rec.spans.size(); ++i) {
        const Span& s = rec.spans[i];
        if (s.bytes == 0) bad("is empty", i);
        if ((size_t)(s.lo - base) % s.align_of != 0) bad("is not aligned for its type", i);
        if (align == 256 && (size_t)(s.lo - base) % 256 != 0) bad("is not 256-byte aligned", i);
        if (s.lo < base || s.lo + s.bytes > base + total) bad("leaves the measured total", i);
        for (size_t j = 0; j < i; ++j)
            if (s.lo < rec.spans[j].lo + rec.spans[j].bytes && rec.spans[j].lo < s.lo + s.bytes) bad("overlaps an earlier one", i);
    }
    if ((size_t)(rec.c.at - base) != total) bad("- measure and carve disagree", rec.spans.size());
    if (total < former || total > former + align * rec.spans.size()) bad("- the total leaves [former, former + align per array]", rec.spans.size());
    printf("%s %d %d %d %zu %zu\n", what, n, b, r, total, former);
    free(base);
}

struct Frag { uint16_t v[8]; };        // stands for the device's 16-byte MFMA operand fragment

}  // namespace

int main() {
    const int Ns[] = {3, 4, 9, 65}, Bs[] = {1, 3}, Rs[] = {1, 3};
    for (int N : Ns)
        for (int B : Bs) {
            const size_t b = (size_t)B, n = (size_t)N, T = (size_t)pfnj::table_len(N), PN = n * (n - 1) / 2;
            pfnj::Staging nj{};
            check("nj", N, B, 0, [&](auto& v) { pfnj::staging_arrays(v, nj, b, N); }, b * T * 8 + b * PN * 4 + b * T * 4 + b);

            float *full, *ctx, *infl, *shift;                       // loo_impl's spans
            check("loo", N, B, 0, [&](auto& v) { pfspan::float_spans(v, {{&full, PN}, {&ctx, PN}, {&infl, n}, {&shift, n}}, b); },
                  b * (2 * PN + 2 * n) * 4);

            for (int R : Rs) {
                const size_t r = (size_t)R;
                if (N >= 4) {
                    const size_t S = n - 3;
                    pfsup::Staging sup{};
                    check("supports", N, B, R, [&](auto& v) { pfsup::staging_arrays(v, sup, b, r, N); },
                          b * S * 8 + b * T * 4 + b * r * T * 4 + 2 * b * S * 4 + b * r + b);
                }
                // place_impl's spans: a backbone of N with Q = R queries
                const size_t M = n + r, PM = M * (M - 1) / 2;
                float *whole, *base, *pl, *dis, *sh, *jt;
                check("place", N, B, R, [&](auto& v) { pfspan::float_spans(v, {{&whole, PM}, {&base, PN}, {&pl, r * n}, {&dis, r}, {&sh, r}, {&jt, r}}, b); },
                      b * (PM + PN + r * n + 3 * r) * 4);

                // pf_mha_forward_device: rows = B R, C = N tokens
                const size_t rows = b * r, C = n, ntiles = (C + 31) / 32;
                Frag *qp, *kp, *vp;
                float* att;
                const size_t qk = pfspan::up(2 * rows * 4 * ntiles * 32 * 2 * 16, 256), vb = pfspan::up(2 * rows * 4 * ntiles * 64 * 16, 256);
                check("mha", N, B, R, [&](auto& v) { pfspan::mha_arrays(v, qp, kp, vp, att, rows, 4, ntiles, C, 64); },
                      2 * qk + vb + pfspan::up(rows * C * 64 * 4, 256), 256);
            }
        }
    const int tiled[][2] = {{5, 2}, {9, 4}, {65, 16}};
    for (const auto& nm : tiled) {
        pftile::Plan p;
        if (!p.build(nm[0], nm[1])) { fprintf(stderr, "pf_staging_main: no plan for N=%d M=%d\n", nm[0], nm[1]); return 1; }
        pftile::Tables t;
        check("tiled", nm[0], nm[1], 0, [&](auto& v) { pftile::table_arrays(v, t, p); }, p.offset.size() * 8 + p.bounds.size() * 4);
    }
    if (!ok) return 1;
    printf("pf_staging_main: clean\n");
    return 0;
}
