// Stand-alone driver of the balanced-SPR bodies of csrc/pf_bme_host.h for AddressSanitizer / UBSan builds
// (tests/test_spr_native.py): run on the CPU thread by thread and workgroup by workgroup, in the order the launches of
// pf_bme.hip.h give them, on exactly-sized heap arrays (pfbme::SprSerial).
//
//     pf_spr_main B N threads epg cap tiled preds.bin start.bin result.bin depth.bin pairs.bin
//
// threads: the size of every workgroup; epg: the target edges one workgroup of the evaluation covers; cap: the moves
// after which a source is capped (-1: step_cap(N)); tiled: 1 = the pair table by the tiled bodies, 0 = one thread
// per entry.  preds.bin: float [B][P_N]; start.bin: int32 [B][T]; result.bin:
// slots int32 [B][T], lengths double [B][T], steps int32 [B], tree_length double [B], status uint8 [B], T = 2 (N - 3)
// + 3; depth.bin: int16 [4N-6][2N-2] and pairs.bin: double [4N-6][4N-6], the first depth and pair table of source 0
// as the bodies built them.
// At every step the depth table the bodies built is compared with build_depth's of the same tree.
// Exit code 0 = done, 2 = usage, 3 = an invalid start table, 4 = a depth table differs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_bme_host.h"

int main(int argc, char** argv) {
    if (argc != 12) return 2;
    const int B = atoi(argv[1]), N = atoi(argv[2]), threads = atoi(argv[3]), epg = atoi(argv[4]);
    const long long cap = atoll(argv[5]);
    const bool tiled = atoi(argv[6]) != 0;
    if (B < 1 || N < 3 || N > 4096 || threads < 1 || epg < 1) return 2;
    const size_t PN = (size_t)N * (N - 1) / 2, T = (size_t)pfnj::table_len(N), b = (size_t)B;
    const size_t nodes = (size_t)pfbme::nodes_of(N), rows = (size_t)pfbme::rows_of(N);
    std::vector<float> preds(b * PN);
    std::vector<int32_t> start(b * T);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(preds.data(), sizeof(float), preds.size(), f) != preds.size()) return 2;
    fclose(f);
    f = fopen(argv[8], "rb");
    if (!f || fread(start.data(), sizeof(int32_t), start.size(), f) != start.size()) return 2;
    fclose(f);

    pfbme::SprSerial run;
    if (!run.setup(preds.data(), start.data(), B, N, epg, cap)) return 3;
    run.tiled = tiled;
    run.init(threads, 2);
    std::vector<int16_t> want(rows * nodes);
    long long tables = 0;
    while (!run.finished())
        for (int step = 0; step < pfbme::ROUND_STEPS; ++step) {
            run.table(false);
            for (size_t s = 0; s < b; ++s) {
                if (pfbme::spr_idle(run.s, s)) continue;
                pfbme::build_depth(&run.parent[s * nodes], &run.children[s * nodes * 3], N, want.data());
                for (size_t i = 0; i < rows * nodes; ++i)
                    if (run.depth[s * rows * nodes + i] != want[i]) {
                        fprintf(stderr, "pf_spr_main: source %zu, row %zu, node %zu: depth %d, build_depth %d\n", s, i / nodes, i % nodes,
                                (int)run.depth[s * rows * nodes + i], (int)want[i]);
                        return 4;
                    }
                ++tables;
            }
            if (tables && step == 0 && run.steps[0] == 0 && !pfbme::spr_idle(run.s, 0)) {
                f = fopen(argv[10], "wb");
                if (!f || fwrite(run.depth.data(), sizeof(int16_t), rows * nodes, f) != rows * nodes) return 2;
                fclose(f);
                f = fopen(argv[11], "wb");
                if (!f || fwrite(run.T.data(), sizeof(double), rows * rows, f) != rows * rows) return 2;
                fclose(f);
            }
            run.evaluate_and_move(threads);
        }
    run.finish(threads);
    std::vector<int32_t> slots(b * T), steps(b);
    std::vector<double> lengths(b * T), tree_length(b);
    std::vector<uint8_t> status(b);
    for (size_t s = 0; s < b; ++s) run.result(s, &slots[s * T], &lengths[s * T], &steps[s], &tree_length[s], &status[s]);

    f = fopen(argv[9], "wb");
    if (!f || fwrite(slots.data(), sizeof(int32_t), slots.size(), f) != slots.size() ||
        fwrite(lengths.data(), sizeof(double), lengths.size(), f) != lengths.size() ||
        fwrite(steps.data(), sizeof(int32_t), steps.size(), f) != steps.size() ||
        fwrite(tree_length.data(), sizeof(double), tree_length.size(), f) != tree_length.size() ||
        fwrite(status.data(), 1, status.size(), f) != status.size())
        return 2;
    fclose(f);
    printf("pf_spr_main: clean, N = %d, rows = %d, depth tables compared = %lld\n", N, 4 * N - 6, tables);
    return 0;
}
