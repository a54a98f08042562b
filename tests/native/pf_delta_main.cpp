// The serial twin of the delta scores (csrc/pf_delta_host.h) as a stand-alone program for AddressSanitizer / UBSan
// (tests/test_delta_host.py builds and runs it; nothing is loaded into Python).
//   pf_delta_main B N K preds.bin result.bin
// preds.bin: float32 [B][P_N].  Every source runs on exactly-sized heap arrays of its own.  result.bin: int64 pair_sum
// [B][P_N], int64 hist [B][K], uint8 flag [B].  Also walks pair_of over every pair of N sequences (the device's decoding
// of a workgroup's pair) and checks it against the enumeration.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_delta_host.h"

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: pf_delta_main B N K preds.bin result.bin\n"); return 2; }
    const int B = std::atoi(argv[1]), N = std::atoi(argv[2]), K = std::atoi(argv[3]);
    if (pfdelta::refused(B, N, K)) { std::printf("refused %d\n", pfdelta::refused(B, N, K)); return 3; }
    const size_t P = (size_t)N * ((size_t)N - 1) / 2;
    std::vector<int64_t> sums((size_t)B * P), hists((size_t)B * (size_t)K);
    std::vector<uint8_t> flags((size_t)B);
    FILE* in = std::fopen(argv[4], "rb");
    if (!in) { std::perror(argv[4]); return 2; }
    for (int b = 0; b < B; ++b) {
        std::unique_ptr<float[]> preds(new float[P]);
        std::unique_ptr<int64_t[]> pair_sum(new int64_t[P]), hist(new int64_t[(size_t)K]);
        std::unique_ptr<uint8_t[]> flag(new uint8_t[1]);
        if (std::fread(preds.get(), sizeof(float), P, in) != P) { std::fprintf(stderr, "short read\n"); return 2; }
        pfdelta::run_serial(preds.get(), N, K, pair_sum.get(), hist.get(), flag.get());
        for (size_t e = 0; e < P; ++e) sums[(size_t)b * P + e] = pair_sum[e];
        for (int k = 0; k < K; ++k) hists[(size_t)b * (size_t)K + (size_t)k] = hist[(size_t)k];
        flags[(size_t)b] = flag[0];
    }
    std::fclose(in);
    int64_t p = 0;
    for (int i = 0; i < N; ++i)
        for (int j = i + 1; j < N; ++j, ++p) {
            int gi = -1, gj = -1;
            pfdelta::pair_of(p, N, &gi, &gj);
            if (gi != i || gj != j) { std::printf("pair_of(%lld) = (%d, %d), not (%d, %d)\n", (long long)p, gi, gj, i, j); return 4; }
        }
    FILE* out = std::fopen(argv[5], "wb");
    if (!out) { std::perror(argv[5]); return 2; }
    std::fwrite(sums.data(), sizeof(int64_t), sums.size(), out);
    std::fwrite(hists.data(), sizeof(int64_t), hists.size(), out);
    std::fwrite(flags.data(), 1, flags.size(), out);
    std::fclose(out);
    std::printf("clean, B = %d, N = %d, K = %d\n", B, N, K);
    return 0;
}
