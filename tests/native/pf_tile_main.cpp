// Stand-alone driver of csrc/pf_tile_host.h for AddressSanitizer / UBSan builds (tests/test_tile_native.py): the plan
// and the body of k_tile_combine, run on the CPU thread by thread on exactly-sized heap arrays.
//
//     pf_tile_main B N M threads sets.bin result.bin
//
// sets.bin: float [B][T]; result.bin: out float [B][P_N], then spread float [B][P_N].  Every output element must be
// written exactly once.  Exit code 0 = done, 2 = usage / bad plan, 3 = an element written twice or never.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_tile_host.h"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int B = atoi(argv[1]), N = atoi(argv[2]), M = atoi(argv[3]), threads = atoi(argv[4]);
    pftile::Plan p;
    if (B < 1 || threads < 1 || !p.build(N, M)) return 2;
    if (p.G != pftile::groups(N, M) || p.bounds[0] != 0 || p.bounds[(size_t)p.G] != N) return 2;
    for (int i = 0; i < N; ++i) {
        const int g = (int)pftile::group_of(N, p.G, i);
        if (g < 0 || g >= p.G || p.bounds[(size_t)g] > i || p.bounds[(size_t)g + 1] <= i) return 2;
    }
    const size_t PN = (size_t)N * (N - 1) / 2, T = (size_t)p.T;
    std::vector<float> sets((size_t)B * T), out((size_t)B * PN), spread((size_t)B * PN);
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(sets.data(), sizeof(float), sets.size(), f) != sets.size()) return 2;
    fclose(f);
    // a NaN of a payload the arithmetic cannot produce marks "not written"
    const uint32_t mark = 0x7fc12345u;
    for (size_t k = 0; k < out.size(); ++k) memcpy(&out[k], &mark, 4), memcpy(&spread[k], &mark, 4);
    const pftile::CombineArgs a{sets.data(), p.bounds.data(), p.offset.data(), out.data(), spread.data(), N, p.G, p.T, (int64_t)PN};
    std::vector<float> seen_out, seen_spread;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i + 1 < N; ++i)
            for (int t = 0; t < threads; ++t) {
                seen_out = out, seen_spread = spread;
                pftile::combine_row(a, i, (size_t)b, t, threads);
                for (size_t k = 0; k < out.size(); ++k) {
                    uint32_t was, is;
                    memcpy(&was, &seen_out[k], 4), memcpy(&is, &out[k], 4);
                    if (was != mark && was != is) return 3;                                     // written twice
                }
            }
    for (size_t k = 0; k < out.size(); ++k) {
        uint32_t o, s;
        memcpy(&o, &out[k], 4), memcpy(&s, &spread[k], 4);
        if (o == mark || s == mark) return 3;                                                  // never written
    }
    f = fopen(argv[6], "wb");
    if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size() ||
        fwrite(spread.data(), sizeof(float), spread.size(), f) != spread.size())
        return 2;
    fclose(f);
    printf("pf_tile_main: clean, G = %d, S = %lld, T = %lld\n", p.G, (long long)p.S, (long long)p.T);
    return 0;
}
