// The serial twin of the least-squares branch lengths (csrc/pf_ols_host.h) as a stand-alone program for AddressSanitizer /
// UBSan (tests/test_ols_host.py builds and runs it; nothing is loaded into Python).
//   pf_ols_main B M N preds.bin slots.bin result.bin
// preds.bin: float32 [B][P_N]; slots.bin: int32 [B][M][T].  Every tree runs on exactly sized heap arrays of its own - the table
// too, so that a table that is none cannot be read past its end unnoticed.  result.bin: float64 ols [B][M][T], uint8 status
// [B][M].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_ols_host.h"

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
    FILE* in = std::fopen(path, "rb");
    if (!in) { std::perror(path); return false; }
    const bool ok = std::fread(v.data(), sizeof(T), v.size(), in) == v.size();
    std::fclose(in);
    if (!ok) std::fprintf(stderr, "short read of %s\n", path);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: pf_ols_main B M N preds.bin slots.bin result.bin\n"); return 2; }
    const int B = std::atoi(argv[1]), M = std::atoi(argv[2]), N = std::atoi(argv[3]);
    if (pfols::refused(B, M, N)) { std::printf("refused %d\n", pfols::refused(B, M, N)); return 3; }
    const size_t n = (size_t)N, P = n * (n - 1) / 2, T = (size_t)pfols::table_len(N), items = (size_t)B * (size_t)M;
    std::vector<float> preds((size_t)B * P);
    std::vector<int32_t> slots(items * T);
    if (!read_all(argv[4], preds) || !read_all(argv[5], slots)) return 2;
    std::vector<double> ols(items * T);
    std::vector<uint8_t> status(items);
    for (size_t item = 0; item < items; ++item) {
        std::unique_ptr<float[]> pred(new float[P]);
        std::unique_ptr<int32_t[]> sl(new int32_t[T]);
        std::unique_ptr<double[]> out(new double[T]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[1]);
        std::memcpy(pred.get(), preds.data() + item / (size_t)M * P, P * sizeof(float));
        std::memcpy(sl.get(), slots.data() + item * T, T * sizeof(int32_t));
        pfols::run_serial(pred.get(), sl.get(), N, out.get(), st.get());
        std::memcpy(ols.data() + item * T, out.get(), T * sizeof(double));
        status[item] = st[0];
    }
    FILE* res = std::fopen(argv[6], "wb");
    if (!res) { std::perror(argv[6]); return 2; }
    std::fwrite(ols.data(), sizeof(double), ols.size(), res);
    std::fwrite(status.data(), 1, status.size(), res);
    std::fclose(res);
    std::printf("clean, B = %d, M = %d, N = %d\n", B, M, N);
    return 0;
}
