// Stand-alone check of the device layouts of the three tree searches for AddressSanitizer / UBSan builds
// (tests/test_tree_layout_native.py): the lists of arrays of csrc/pf_nj_host.h and csrc/pf_bme_host.h (neighbour
// joining, balanced NNI, balanced SPR) under their three visitors.
//
//     pf_layout_main
//
// For N in {3, 4, 9, 65, 137, 300} and B in {1, 3}, per state: carve B sources from an 8-byte aligned base, record every
// array a fourth visitor sees behind the carving one, and check that
//   - every span starts 8-byte aligned (the one-byte flags of a source share one span: the span is checked, and every
//     flag array lies inside it),
//   - the arrays are pairwise disjoint,
//   - all of them lie inside B * state_bytes(N),
//   - for B = 1 the measured bytes are the carved extent.
// Prints "<state> <N> <bytes per source>" per state and N.  Exit code 0 = all hold, 1 = one does not (named on stderr).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_bme_host.h"

namespace {

struct Span { const char* lo; size_t bytes; bool aligned_start; };

// carves, and keeps what it handed out
struct Record {
    pfnj::Carve c;
    std::vector<Span> spans;
    template <class T> void operator()(T*& p, size_t count) {
        c(p, count);
        spans.push_back({reinterpret_cast<const char*>(p), count * sizeof(T), true});
    }
    void flags(size_t B, std::initializer_list<uint8_t**> list) {
        const char* span = c.at;
        c.flags(B, list);
        bool first = true;
        for (uint8_t** p : list) {
            // the span's start is the first flag array; the others follow inside its 8 B bytes
            if (reinterpret_cast<const char*>(*p) < span || reinterpret_cast<const char*>(*p) + B > span + 8 * B) {
                fprintf(stderr, "a flag array leaves its span\n");
                exit(1);
            }
            spans.push_back({reinterpret_cast<const char*>(*p), B, first});
            first = false;
        }
    }
};

bool check(const char* state, int N, int B, const char* base, size_t per, const Record& r, size_t measured_b1) {
    const size_t extent = (size_t)(r.c.at - base);
    bool ok = true;
    auto bad = [&](const char* what, size_t i) {
        fprintf(stderr, "pf_layout_main: %s N=%d B=%d: array %zu %s\n", state, N, B, i, what);
        ok = false;
    };
    for (size_t i = 0; i < r.spans.size(); ++i) {
        const Span& s = r.spans[i];
        if (s.bytes == 0) bad("is empty", i);
        if (s.aligned_start && (size_t)(s.lo - base) % 8 != 0) bad("is not 8-byte aligned", i);
        if (s.lo < base || s.lo + s.bytes > base + (size_t)B * per) bad("leaves B * state_bytes(N)", i);
        for (size_t j = 0; j < i; ++j)
            if (s.lo < r.spans[j].lo + r.spans[j].bytes && r.spans[j].lo < s.lo + s.bytes) bad("overlaps an earlier one", i);
    }
    if (extent > (size_t)B * per) bad("- the carved extent exceeds B * state_bytes(N)", r.spans.size());
    if (B == 1 && (extent != per || measured_b1 != per)) bad("- measure and carve disagree for B = 1", r.spans.size());
    return ok;
}

}  // namespace

int main() {
    const int Ns[] = {3, 4, 9, 65, 137, 300}, Bs[] = {1, 3};
    bool ok = true;
    for (int N : Ns) {
        const size_t per_nj = pfnj::state_bytes(N), per_nni = pfbme::state_bytes(N), per_spr = pfbme::spr_state_bytes(N);
        printf("nj %d %zu\nbnni %d %zu\nspr %d %zu\n", N, per_nj, N, per_nni, N, per_spr);
        for (int B : Bs) {
            // exactly B * state_bytes(N) bytes each (never written: the layout alone is looked at)
            std::vector<double> ws_nj(B * per_nj / 8), ws_nni(B * per_nni / 8), ws_spr(B * per_spr / 8);
            if (per_nj % 8 || per_nni % 8 || per_spr % 8) { fprintf(stderr, "pf_layout_main: N=%d: bytes per source not a multiple of 8\n", N); return 1; }

            char* base = reinterpret_cast<char*>(ws_nj.data());
            pfnj::Args a = pfnj::args_of(nullptr, N, pfnj::Q_GROUPS, nullptr, nullptr, nullptr);
            pfnj::Measure m_nj;
            pfnj::state_arrays(m_nj, a, 1);
            Record r_nj{{base}, {}};
            pfnj::state_arrays(r_nj, a, (size_t)B);
            const pfnj::Args a2 = pfnj::carve(base, nullptr, B, N, nullptr, nullptr, nullptr);
            if (a2.d != a.d || a2.r != a.r || a2.part != a.part || a2.active != a.active) { fprintf(stderr, "pf_layout_main: pfnj::carve differs from its list\n"); return 1; }
            ok &= check("nj", N, B, base, per_nj, r_nj, m_nj.bytes);

            base = reinterpret_cast<char*>(ws_nni.data());
            pfbme::Args b = pfbme::args_of(nullptr, N, pfbme::eval_groups(N, pfbme::EVAL_EDGES));
            pfnj::Measure m_nni;
            pfbme::state_arrays(m_nni, b, 1);
            Record r_nni{{base}, {}};
            pfbme::state_arrays(r_nni, b, (size_t)B);
            const pfbme::Args b2 = pfbme::carve(base, nullptr, B, N);
            if (b2.d != b.d || b2.depth != b.depth || b2.move != b.move || b2.status != b.status || b2.part_cap != b.part_cap) {
                fprintf(stderr, "pf_layout_main: pfbme::carve differs from its list\n");
                return 1;
            }
            ok &= check("bnni", N, B, base, per_nni, r_nni, m_nni.bytes);

            base = reinterpret_cast<char*>(ws_spr.data());
            pfbme::SprArgs s = pfbme::carve_spr(base, nullptr, B, N, 0);         // (its scalars; carved again below)
            pfnj::Measure m_spr;
            pfbme::spr_state_arrays(m_spr, s, 1);
            const pfbme::SprArgs s2 = s;
            Record r_spr{{base}, {}};
            pfbme::spr_state_arrays(r_spr, s, (size_t)B);
            if (s2.T != s.T || s2.spart != s.spart || s2.path != s.path || s2.sdone != s.sdone || s2.b.depth != s.b.depth) {
                fprintf(stderr, "pf_layout_main: pfbme::carve_spr differs from its list\n");
                return 1;
            }
            ok &= check("spr", N, B, base, per_spr, r_spr, m_spr.bytes);
        }
    }
    if (!ok) return 1;
    printf("pf_layout_main: clean\n");
    return 0;
}
