// Stand-alone driver of csrc/pf_bionj_host.h for AddressSanitizer / UBSan builds (tests/test_bionj_native.py): the
// bodies of the BIONJ kernels, run on the CPU thread by thread and workgroup by workgroup, in the order the launches of
// pf_bionj.hip.h give them, on exactly-sized heap arrays.
//
//     pf_bionj_main B N threads groups preds.bin result.bin
//
// threads: the size of every workgroup; groups: the most workgroups of the two minima (min(m, groups) run).
// preds.bin: float [B][P_N]; result.bin: slots int32 [B][T], then lengths double [B][T], then flag uint8 [B],
// T = 2 (N - 3) + 3.  Exit code 0 = done, 2 = usage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_bionj_host.h"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int B = atoi(argv[1]), N = atoi(argv[2]), threads = atoi(argv[3]), groups = atoi(argv[4]);
    if (B < 1 || N < 3 || N > 4096 || threads < 1 || groups < 1) return 2;
    const size_t PN = (size_t)N * (N - 1) / 2, T = (size_t)pfnj::table_len(N), b = (size_t)B;
    std::vector<float> preds(b * PN);
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(preds.data(), sizeof(float), preds.size(), f) != preds.size()) return 2;
    fclose(f);
    std::vector<double> lengths(b * T);
    std::vector<int32_t> slots(b * T);
    std::vector<uint8_t> flag(b, 0);
    std::vector<pfnj::Key> keys((size_t)threads);
    pfbionj::Args a = pfbionj::args_of(preds.data(), N, groups, slots.data(), lengths.data(), flag.data());
    pfspan::Allocate mem;                                // d, r, part, active, v, part_at, label: one exactly sized allocation each
    pfbionj::state_arrays(mem, a, b);

    const int init_groups = 2;
    for (size_t src = 0; src < b; ++src)
        for (int wg = 0; wg < init_groups; ++wg)
            for (int tid = 0; tid < threads; ++tid) pfbionj::init_elems(a, src, wg, init_groups, tid, threads);
    for (int t = 0; t < N - 3; ++t) {
        const int m = N - t, G = m < groups ? m : groups;
        for (size_t src = 0; src < b; ++src)
            for (int row = 0; row < m; ++row) pfnj::row_sum(a.nj, m, t, src, row);
        for (size_t src = 0; src < b; ++src)
            for (int wg = 0; wg < G; ++wg) {
                for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = pfbionj::qmin_thread(a, m, t, src, wg, G, tid, threads);
                pfnj::reduce_keys_serial(keys.data(), threads);
                a.nj.part[src * (size_t)groups + (size_t)wg] = keys[0];
            }
        for (size_t src = 0; src < b; ++src)
            for (int wg = 0; wg < G; ++wg) {
                for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = pfbionj::part_thread_key(a, a.nj.part, src, G, tid, threads);
                pfnj::reduce_keys_serial(keys.data(), threads);
                const double qstar = keys[0].v;
                for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = pfbionj::pick_thread(a, m, t, src, qstar, wg, G, tid, threads);
                pfnj::reduce_keys_serial(keys.data(), threads);
                a.part_at[src * (size_t)groups + (size_t)wg] = keys[0];
            }
        for (size_t src = 0; src < b; ++src) {
            for (int tid = 0; tid < threads; ++tid) keys[(size_t)tid] = pfbionj::part_thread_key(a, a.part_at, src, G, tid, threads);
            pfnj::reduce_keys_serial(keys.data(), threads);
            const pfbionj::Join j = pfbionj::join_record(a, m, t, src, keys[0]);
            for (int tid = 0; tid < threads; ++tid) pfbionj::join_update(a, m, t, src, j, tid, threads);
        }
    }
    for (size_t src = 0; src < b; ++src) pfbionj::final_record(a, src);

    f = fopen(argv[6], "wb");
    if (!f || fwrite(slots.data(), sizeof(int32_t), slots.size(), f) != slots.size() ||
        fwrite(lengths.data(), sizeof(double), lengths.size(), f) != lengths.size() ||
        fwrite(flag.data(), 1, flag.size(), f) != flag.size())
        return 2;
    fclose(f);
    printf("pf_bionj_main: clean, N = %d, joins = %d\n", N, N - 3);
    return 0;
}
