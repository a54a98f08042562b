// Stand-alone driver of csrc/pf_bme_host.h for AddressSanitizer / UBSan builds (tests/test_bme_native.py): the bodies of
// the balanced-NNI kernels, run on the CPU thread by thread and workgroup by workgroup, in the order the launches of
// pf_bme.hip.h give them, on exactly-sized heap arrays (pfbme::Serial).
//
//     pf_bme_main B N threads epg preds.bin start.bin result.bin
//
// threads: the size of every workgroup; epg: the edges one workgroup of the evaluation covers.  preds.bin: float
// [B][P_N]; start.bin: int32 [B][T], the slots of the start tables; result.bin: slots int32 [B][T], lengths double
// [B][T], steps int32 [B], tree_length double [B], status uint8 [B], T = 2 (N - 3) + 3.
// Exit code 0 = done, 2 = usage, 3 = an invalid start table.  The last line names the from-scratch tables that offered
// a move the incrementally updated table had not (resumes).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_bme_host.h"

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int B = atoi(argv[1]), N = atoi(argv[2]), threads = atoi(argv[3]), epg = atoi(argv[4]);
    if (B < 1 || N < 3 || N > 4096 || threads < 1 || epg < 1) return 2;
    const size_t PN = (size_t)N * (N - 1) / 2, T = (size_t)pfnj::table_len(N), b = (size_t)B;
    std::vector<float> preds(b * PN);
    std::vector<int32_t> start(b * T);
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(preds.data(), sizeof(float), preds.size(), f) != preds.size()) return 2;
    fclose(f);
    f = fopen(argv[6], "rb");
    if (!f || fread(start.data(), sizeof(int32_t), start.size(), f) != start.size()) return 2;
    fclose(f);

    pfbme::Serial run;
    if (!run.setup(preds.data(), start.data(), B, N, epg)) return 3;
    run.run(threads, epg, 2);
    std::vector<int32_t> slots(b * T), steps(b);
    std::vector<double> lengths(b * T), tree_length(b);
    std::vector<uint8_t> status(b);
    for (size_t s = 0; s < b; ++s) run.result(s, &slots[s * T], &lengths[s * T], &steps[s], &tree_length[s], &status[s]);

    f = fopen(argv[7], "wb");
    if (!f || fwrite(slots.data(), sizeof(int32_t), slots.size(), f) != slots.size() ||
        fwrite(lengths.data(), sizeof(double), lengths.size(), f) != lengths.size() ||
        fwrite(steps.data(), sizeof(int32_t), steps.size(), f) != steps.size() ||
        fwrite(tree_length.data(), sizeof(double), tree_length.size(), f) != tree_length.size() ||
        fwrite(status.data(), 1, status.size(), f) != status.size())
        return 2;
    fclose(f);
    printf("pf_bme_main: clean, N = %d, edges = %d, resumes = %lld\n", N, 2 * N - 3, (long long)run.resumes);
    return 0;
}
