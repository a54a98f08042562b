// Stand-alone check of the staging lists for AddressSanitizer / UBSan builds (tests/test_staging_native.py): what the host
// entry points carve from one grow-only device buffer each, described once per layout and driven by the visitors of
// csrc/pf_spans.h - the staging of pf_nj_joins (pf_nj_host.h), of pf_join_supports and pf_join_transfers
// (pf_support_host.h) and of pf_join_consensus (pf_consensus_host.h), the two tables of the tiling plan (pf_tile_host.h),
// the float spans of leave-one-out and of placement (pf_lib.hip hands them to pfspan::float_spans as they stand here),
// and the workspace of the attention operator (pfspan::mha_arrays).
//
//     pf_staging_main
//
// For every list and shape: measure it, carve it from a buffer of exactly that many bytes (aligned as a device
// allocation is), record every array behind the carving visitor, and check that
//   - every array is aligned for its element type,
//   - every array lies inside the measured total,
//   - the arrays are pairwise disjoint,
//   - no array is empty but those the list declares absent, and those are the ones the variant does without
//     (transfers without branch_moves: 1; consensus without lengths: 3),
//   - the total is at most 8 bytes per array (256 for the attention operator) above the formula the layout had when
//     it was a chain of byte offsets (transfers, consensus: the plain sum of the arrays' bytes), and not below it.
// The four calls' lists also make a round trip through pfspan::upload / download with memcpy as the copy ("trip" lines):
// the caller's arrays are exactly sized allocations of the shapes include/phyloformer_amd.h documents - not of the
// list's counts, so a count that disagrees with the header is a red-zone hit or a pattern that does not arrive -, the
// staging one exactly sized allocation.  Every input carries a pattern of its own up, every result one down; no input is
// written, an optional array passed as null stays null in the staging.
// Shapes: N in {3, 4, 9, 65} (supports, transfers, consensus: N >= 4, a tree of 3 has no split), chunk or B in {1, 3},
// R or Q in {1, 3}; the tiling plans of (N, M) = (5, 2), (9, 4), (65, 16).  The odd counts leave the narrow arrays off
// alignment.  Exit code 0 = all hold, 1 = one does not (named on stderr).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_consensus_host.h"
#include "../../phyloformer_amd/csrc/pf_nj_host.h"
#include "../../phyloformer_amd/csrc/pf_support_host.h"
#include "../../phyloformer_amd/csrc/pf_tile_host.h"

namespace {

struct Span { const char* lo; size_t bytes, align_of; bool absent; };

// carves, and keeps what it handed out
struct Record {
    pfspan::Carve c;
    std::vector<Span> spans;
    template <class T> void operator()(T*& p, size_t count) {
        c(p, count);
        spans.push_back({reinterpret_cast<const char*>(p), count * sizeof(T), alignof(T), false});
    }
    template <class T> void in(const T*& p, const T* callers, size_t count, pfspan::Need need = pfspan::REQUIRED) {
        spans.push_back({c.at, need == pfspan::ABSENT ? 0 : count * sizeof(T), alignof(T), need == pfspan::ABSENT});
        c.in(p, callers, count, need);
    }
    template <class T> void out(T*& p, T* callers, size_t count, pfspan::Need need = pfspan::REQUIRED) {
        spans.push_back({c.at, need == pfspan::ABSENT ? 0 : count * sizeof(T), alignof(T), need == pfspan::ABSENT});
        c.out(p, callers, count, need);
    }
};

bool ok = true;

// `former`: the bytes of the offset chain
template <class List>
void check(const char* what, int n, int b, int r, List&& list, size_t former, size_t align = 8, size_t absent = 0) {
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
        if (s.bytes == 0 && !s.absent) bad("is empty", i);
        if (s.absent) --absent;
        if ((size_t)(s.lo - base) % s.align_of != 0) bad("is not aligned for its type", i);
        if (align == 256 && (size_t)(s.lo - base) % 256 != 0) bad("is not 256-byte aligned", i);
        if (s.lo < base || s.lo + s.bytes > base + total) bad("leaves the measured total", i);
        for (size_t j = 0; j < i; ++j)
            if (s.lo < rec.spans[j].lo + rec.spans[j].bytes && rec.spans[j].lo < s.lo + s.bytes) bad("overlaps an earlier one", i);
    }
    if (absent != 0) bad("- the list declares other arrays absent than the variant does without", rec.spans.size());
    if ((size_t)(rec.c.at - base) != total) bad("- measure and carve disagree", rec.spans.size());
    if (total < former || total > former + align * rec.spans.size()) bad("- the total leaves [former, former + align per array]", rec.spans.size());
    printf("%s %d %d %d %zu %zu\n", what, n, b, r, total, former);
    free(base);
}

// ---- the round trip of a call's list through pfspan::upload / download ------------------------------------------------

// byte i of the pattern of array k (never FILL, what the staging holds before anything arrives)
const unsigned char FILL = 0x5a;
unsigned char pattern(size_t k, size_t i) {
    const unsigned char v = (unsigned char)(k * 37 + i * 11 + 1);
    return v == FILL ? (unsigned char)(FILL + 1) : v;
}
template <class T> unsigned char* bytes_of(const T* p) { return const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(p)); }
void fill(unsigned char* p, size_t k, size_t bytes) { for (size_t i = 0; i < bytes; ++i) p[i] = pattern(k, i); }
bool holds(const unsigned char* p, size_t k, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i)
        if (p[i] != pattern(k, i)) return false;
    return true;
}

// a caller's array of `count` elements: an allocation of exactly its bytes
template <class T> T* fresh(pfspan::Allocate& mem, size_t count) { T* p; mem(p, count); return p; }

// `arrays(f)` calls f(staging pointer, caller's pointer, elements, is it an input?) for every array of the call, with
// the elements of its documented shape; the caller's arrays are allocated already (a null one: not passed).
template <class List, class Arrays>
void round_trip(const char* what, int n, int b, int r, List&& list, Arrays&& arrays) {
    auto bad = [&](const char* why, size_t k) {
        fprintf(stderr, "pf_staging_main: trip %s N=%d B=%d R=%d: array %zu %s\n", what, n, b, r, k, why);
        ok = false;
    };
    auto copy = [](void* to, const void* from, size_t bytes) { memcpy(to, from, bytes); return 0; };
    size_t k = 0, moved = 0;
    arrays([&](auto* staged, auto* callers, size_t count, bool input) {        // inputs: their pattern; results: FILL
        (void)staged;
        if (callers && input) fill(bytes_of(callers), k, count * sizeof(*callers));
        else if (callers) memset(bytes_of(callers), FILL, count * sizeof(*callers));
        ++k;
    });
    const size_t total = pfspan::measure(list);
    pfspan::Allocate mem;
    unsigned char* base = fresh<unsigned char>(mem, total);
    memset(base, FILL, total);
    pfspan::carve(reinterpret_cast<char*>(base), list);
    if (pfspan::missing(list)) bad("- a required pointer counts as null", 0);
    if (pfspan::upload(list, copy) != 0) bad("- upload failed", 0);
    k = 0;
    arrays([&](auto* staged, auto* callers, size_t count, bool input) {
        const size_t bytes = count * sizeof(*callers);
        if ((staged == nullptr) != (callers == nullptr)) bad("is in the staging and not with the caller, or the reverse", k);
        else if (staged && input && !holds(bytes_of(staged), k, bytes)) bad("did not arrive in the staging", k);
        else if (staged && !input) fill(bytes_of(staged), k + 100, bytes);
        ++k;
    });
    if (pfspan::download(list, copy) != 0) bad("- download failed", 0);
    k = 0;
    arrays([&](auto* staged, auto* callers, size_t count, bool input) {
        (void)staged;
        if (callers && !holds(bytes_of(callers), input ? k : k + 100, count * sizeof(*callers)))
            bad(input ? "was written, an input" : "did not arrive with the caller", k);
        if (callers) moved += count * sizeof(*callers);
        ++k;
    });
    printf("trip %s %d %d %d %zu %zu\n", what, n, b, r, k, moved);
}

struct Frag { uint16_t v[8]; };        // stands for the device's 16-byte MFMA operand fragment

}  // namespace

int main() {
    const int Ns[] = {3, 4, 9, 65}, Bs[] = {1, 3}, Rs[] = {1, 3};
    for (int N : Ns)
        for (int B : Bs) {
            const size_t b = (size_t)B, n = (size_t)N, T = (size_t)pfnj::table_len(N), PN = n * (n - 1) / 2;
            {
                pfspan::Allocate mem;
                pfnj::Tables nj{};
                const pfnj::Tables u{fresh<float>(mem, b * PN), fresh<int32_t>(mem, b * T), fresh<double>(mem, b * T), fresh<uint8_t>(mem, b)};
                auto list = [&](auto& v) { pfnj::staging_arrays(v, nj, u, b, N); };
                check("nj", N, B, 0, list, b * T * 8 + b * PN * 4 + b * T * 4 + b);
                round_trip("nj", N, B, 0, list, [&](auto&& f) {
                    f(nj.preds, u.preds, b * PN, true); f(nj.slots, u.slots, b * T, false); f(nj.lengths, u.lengths, b * T, false);
                    f(nj.flag, u.flag, b, false);
                });
            }

            float *full, *ctx, *infl, *shift;                       // loo_impl's spans
            check("loo", N, B, 0, [&](auto& v) { pfspan::float_spans(v, {{&full, PN}, {&ctx, PN}, {&infl, n}, {&shift, n}}, b); },
                  b * (2 * PN + 2 * n) * 4);

            for (int R : Rs) {
                const size_t r = (size_t)R;
                if (N >= 4) {
                    const size_t S = n - 3;
                    // variant 0: pf_join_supports; 1, 2: pf_join_transfers without and with branch_moves; a rep_flag
                    // in variants 0 and 2
                    for (int variant = 0; variant < 3; ++variant) {
                        const bool transfers = variant > 0, branch = variant == 2, flag = variant != 1;
                        const char* const what = transfers ? "transfers" : "supports";
                        pfspan::Allocate mem;
                        pfsup::Tables sup{}, u{};
                        u.ref = fresh<int32_t>(mem, b * T); u.rep = fresh<int32_t>(mem, b * r * T);
                        u.flag = flag ? fresh<uint8_t>(mem, b * r) : nullptr;
                        u.count = fresh<int32_t>(mem, b * S); u.transfer = fresh<int64_t>(mem, b * S); u.depth = fresh<int32_t>(mem, b * S);
                        u.status = fresh<uint8_t>(mem, b);
                        if (transfers) {
                            u.moves = fresh<int64_t>(mem, b * n); u.used = fresh<int32_t>(mem, b * S); u.capped = fresh<int32_t>(mem, b * S);
                            u.branch = branch ? fresh<int32_t>(mem, b * S * n) : nullptr;
                        }
                        auto list = [&](auto& v) { pfsup::staging_arrays(v, sup, u, b, r, N, transfers, branch); };
                        const size_t former = b * S * 8 + b * T * 4 + b * r * T * 4 + 2 * b * S * 4 + b * r + b;
                        if (!transfers) check(what, N, B, R, list, former);
                        else check(what, N, B, R, list, former + b * n * 8 + 2 * b * S * 4 + (branch ? b * S * n * 4 : 0), 8, branch ? 0 : 1);
                        round_trip(what, N, B, R, list, [&](auto&& f) {
                            f(sup.ref, u.ref, b * T, true); f(sup.rep, u.rep, b * r * T, true); f(sup.flag, u.flag, b * r, true);
                            f(sup.count, u.count, b * S, false); f(sup.transfer, u.transfer, b * S, false); f(sup.depth, u.depth, b * S, false);
                            f(sup.status, u.status, b, false);
                            if (!transfers) return;
                            f(sup.moves, u.moves, b * n, false); f(sup.used, u.used, b * S, false); f(sup.capped, u.capped, b * S, false);
                            f(sup.branch, u.branch, b * S * n, false);
                        });
                    }
                    // pf_join_consensus without and with lengths; a rep_flag with them
                    for (int lengths = 0; lengths < 2; ++lengths) {
                        pfspan::Allocate mem;
                        pfcon::Tables con{}, u{};
                        u.rep = fresh<int32_t>(mem, b * r * T);
                        u.lengths = lengths ? fresh<double>(mem, b * r * T) : nullptr;
                        u.flag = lengths ? fresh<uint8_t>(mem, b * r) : nullptr;
                        u.n_splits = fresh<int32_t>(mem, b); u.count = fresh<int32_t>(mem, b * S); u.size = fresh<int32_t>(mem, b * S);
                        u.parent = fresh<int32_t>(mem, b * S); u.leaf_parent = fresh<int32_t>(mem, b * n);
                        u.split_length = lengths ? fresh<double>(mem, b * S) : nullptr;
                        u.leaf_length = lengths ? fresh<double>(mem, b * n) : nullptr;
                        u.status = fresh<uint8_t>(mem, b);
                        auto list = [&](auto& v) { pfcon::staging_arrays(v, con, u, b, r, N); };
                        const size_t with = lengths ? b * r * T * 8 + b * S * 8 + b * n * 8 : 0;
                        check("consensus", N, B, R, list, with + b * r * T * 4 + b * 4 + 3 * b * S * 4 + b * n * 4 + b * r + b, 8, lengths ? 0 : 3);
                        round_trip("consensus", N, B, R, list, [&](auto&& f) {
                            f(con.rep, u.rep, b * r * T, true); f(con.lengths, u.lengths, b * r * T, true); f(con.flag, u.flag, b * r, true);
                            f(con.n_splits, u.n_splits, b, false); f(con.count, u.count, b * S, false); f(con.size, u.size, b * S, false);
                            f(con.parent, u.parent, b * S, false); f(con.split_length, u.split_length, b * S, false);
                            f(con.leaf_parent, u.leaf_parent, b * n, false); f(con.leaf_length, u.leaf_length, b * n, false);
                            f(con.status, u.status, b, false);
                        });
                    }
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
