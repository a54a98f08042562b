// Stand-alone walk of the default kernels' workspace list (csrc/pf_host_prep.h: workspace_arrays) under the visitors of
// csrc/pf_spans.h, against the offset chain the list replaced, kept here verbatim as the "former" layout.  For every
// shape: each array's offset and the total equal the former's; each array is 256-aligned, inside the total and disjoint
// from the others; the 32-token trash area behind x, qrow and qcol lies inside their spans at token B P Lloc; the four
// int arrays share one span, cut srep | ulist | ucount | plan.  Offsets are recorded by a visitor (no base pointer is
// invented); the int span alone is given real, exactly sized memory, so the cut is checked under the sanitizers.
// Prints one line per shape, "ws <B> <N> <Lloc> <fine> <tile_force> <total> <former>", and "pf_workspace_main: clean".
#include <cstdio>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_host_prep.h"
#include "../../phyloformer_amd/csrc/pf_spans.h"

using namespace pfhost;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ---- the former layout: pf_lib.hip's workspace_bytes as it stood (CPART = 4 * 64 + 8 in pf_device.hip.h) ---------------
constexpr int WS_BUFS = 12, CPART = 4 * 64 + 8;
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static size_t former_bytes(int colstats_fine, int tile_force, int B, int P, int Lloc, size_t off[WS_BUFS]) {
    Lloc = std::max(Lloc, 1);
    const ColPlan c = colstats_plan_core(B, P, Lloc, colstats_fine);
    const int nparts = c.fine ? c.G * c.S : c.G;
    const size_t tok = (size_t)B * P * Lloc;
    size_t o = 0;
    off[0] = o; o = align_up(o + (tok + 32) * 64 * 4, 256);              // x (+ 32-token trash area)
    off[1] = o; o = align_up(o + (tok + 32) * 4 * 4, 256);               // qrow (+ trash)
    off[2] = o; o = align_up(o + (tok + 32) * 4 * 4, 256);               // qcol (+ trash)
    off[3] = o; o = align_up(o + (size_t)B * P * SROW * 4, 256);         // srow
    off[4] = o; o = align_up(o + (size_t)B * P * MROW * 4, 256);         // mrow
    off[5] = o; o = align_up(o + (size_t)B * nparts * Lloc * CPART * 4, 256); // part
    off[6] = o; o = align_up(o + (size_t)B * Lloc * 64 * 4, 256);        // ctx
    off[7] = o; o = align_up(o + (size_t)B * P * MFRAG_PER_PAIR * 16, 256); // mfrag
    const size_t slots = (size_t)tile_plan_core(P, Lloc, tile_force).slots_aln;
    off[8] = o; o = align_up(o + (size_t)B * slots * SROW * 4, 256);   // spart: row statistics per tile part
    off[9] = o; o = align_up(o + (size_t)B * slots * 4, 256);          // outpart: head sums per tile part
    off[10] = o; o = align_up(o + (size_t)B * P * 4 * 4, 256);         // rq: L / S_q per pair and head
    off[11] = o; o = align_up(o + ((size_t)B * Lloc * 2 + B + main_plan_ints(B)) * sizeof(int), 256);   // srep | ulist | ucount | plan
    return o;
}

// Where Carve would put each array, as numbers; an int array also gets memory of exactly its size.
struct Record {
    struct Span { const void* field; size_t off, bytes; };
    std::vector<Span> spans;
    std::vector<std::unique_ptr<int[]>> owned;
    size_t at = 0;
    template <class T> void operator()(T*& p, size_t count) {
        spans.push_back({&p, at, count * sizeof(T)});
        at += pfspan::up(count * sizeof(T), 256);
        if constexpr (std::is_same<T, int>::value) { owned.emplace_back(new int[count]()); p = owned.back().get(); }
    }
};

static void check(int B, int N, int Lloc, int fine, int tile_force) {
    const int P = N * (N - 1) / 2;
    size_t off[WS_BUFS];
    const size_t former = former_bytes(fine, tile_force, B, P, Lloc, off);
    Workspace w, wm;
    Record rec;
    workspace_arrays(rec, w, B, P, Lloc, fine, tile_force);
    const size_t total = pfspan::measure([&](auto& v) { workspace_arrays(v, wm, B, P, Lloc, fine, tile_force); }, 256);
    std::printf("ws %d %d %d %d %d %zu %zu\n", B, N, Lloc, fine, tile_force, total, former);
    char at[96];
    std::snprintf(at, sizeof at, "B %d N %d Lloc %d fine %d force %d", B, N, Lloc, fine, tile_force);
    CHECK(total == former && rec.at == former, "%s", at);
    CHECK(wm.srep == nullptr && wm.ulist == nullptr && wm.plan == nullptr && wm.x == nullptr, "%s", at);   // measuring carves nothing
    const ColPlan c = colstats_plan_core(B, P, std::max(Lloc, 1), fine);
    CHECK(w.G == c.G && w.sub == c.sub && w.S == c.S && w.fine == c.fine && wm.G == c.G && wm.fine == c.fine, "%s", at);
    // the former's order: x qrow qcol srow mrow part ctx mfrag spart outpart rq ints
    const void* order[WS_BUFS] = {&w.x, &w.qrow, &w.qcol, &w.srow, &w.mrow, &w.part, &w.ctx, &w.mfrag, &w.spart, &w.outpart, &w.rq, &w.srep};
    CHECK(rec.spans.size() == (size_t)WS_BUFS, "%s", at);
    if (rec.spans.size() != (size_t)WS_BUFS) return;
    for (int i = 0; i < WS_BUFS; ++i) {
        const Record::Span& s = rec.spans[i];
        CHECK(s.field == order[i] && s.off == off[i], "%s: array %d at %zu, formerly %zu", at, i, s.off, off[i]);
        CHECK(s.off % 256 == 0 && s.bytes > 0 && s.off + s.bytes <= total, "%s: array %d", at, i);
        for (int j = 0; j < i; ++j)
            CHECK(rec.spans[j].off + rec.spans[j].bytes <= s.off, "%s: arrays %d and %d overlap", at, j, i);
    }
    // the trash area: 32 tokens from token B P Lloc (MainArgs::trash_tok) of x (64 floats a token), qrow and qcol (4)
    const size_t trash_tok = (size_t)B * P * Lloc;
    CHECK((trash_tok + 32) * 64 * 4 <= rec.spans[0].bytes, "%s", at);
    CHECK((trash_tok + 32) * 4 * 4 <= rec.spans[1].bytes && (trash_tok + 32) * 4 * 4 <= rec.spans[2].bytes, "%s", at);
    // the int span: srep [B][Lloc] | ulist [B][Lloc] | ucount [B] | plan [main_plan_ints(B)], an empty shard as one site
    const size_t sites = (size_t)B * std::max(Lloc, 1), ints = rec.spans[11].bytes / sizeof(int);
    CHECK(w.ulist == w.srep + sites && w.ucount == w.ulist + sites && w.plan == w.ucount + B, "%s", at);
    CHECK(w.plan + pfk::main_plan_ints(B) == w.srep + ints, "%s", at);
    for (size_t i = 0; i < sites; ++i) { w.srep[i] = 1; w.ulist[i] = 2; }
    for (int i = 0; i < B; ++i) w.ucount[i] = 3;
    for (int i = 0; i < pfk::main_plan_ints(B); ++i) w.plan[i] = 4;
    size_t sum = 0;
    for (size_t i = 0; i < ints; ++i) sum += (size_t)w.srep[i];
    CHECK(sum == 3 * sites + 3 * (size_t)B + 4 * (size_t)pfk::main_plan_ints(B), "%s", at);
}

int main() {
    static_assert(WS_CPART == CPART, "the list's partial size is the former chain's");
    for (int B : {1, 2, 3, 17})
        for (int N : {2, 3, 20, 200})
            for (int Lloc : {0, 1, 31, 32, 33, 500, 4096})
                for (int fine : {-1, 0, 1})
                    for (int tile_force : {-1, 0, 1})      // tile_plan_core tells 0, 1 and anything else apart
                        check(B, N, Lloc, fine, tile_force);
    if (fails) { std::printf("pf_workspace_main: %d failures\n", fails); return 1; }
    std::printf("pf_workspace_main: clean\n");
    return 0;
}
