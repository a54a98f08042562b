// The serial twin of the tree fit (csrc/pf_fit_host.h) as a stand-alone program for AddressSanitizer / UBSan
// (tests/test_fit_host.py builds and runs it; nothing is loaded into Python).
//   pf_fit_main B M N keep preds.bin slots.bin lengths.bin result.bin
// preds.bin: float32 [B][P_N]; slots.bin: int32 [B][M][T]; lengths.bin: float64 [B][M][T].  Every tree runs on exactly sized
// heap arrays of its own - the tables too, so that a table that is none cannot be read past its end unnoticed.  keep = 1:
// with the patristic array, 0: without (run_serial keeps the distances itself).  result.bin: float64 patristic [B][M][P_N]
// (keep = 1 only), float64 rows [B][M][N][6], int32 worst_j [B][M][N], uint8 status [B][M].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_fit_host.h"

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
    if (argc != 9) { std::fprintf(stderr, "usage: pf_fit_main B M N keep preds.bin slots.bin lengths.bin result.bin\n"); return 2; }
    const int B = std::atoi(argv[1]), M = std::atoi(argv[2]), N = std::atoi(argv[3]), keep = std::atoi(argv[4]);
    if (pffit::refused(B, M, N)) { std::printf("refused %d\n", pffit::refused(B, M, N)); return 3; }
    const size_t n = (size_t)N, P = n * (n - 1) / 2, T = (size_t)pffit::table_len(N), items = (size_t)B * (size_t)M;
    std::vector<float> preds((size_t)B * P);
    std::vector<int32_t> slots(items * T);
    std::vector<double> lengths(items * T);
    if (!read_all(argv[5], preds) || !read_all(argv[6], slots) || !read_all(argv[7], lengths)) return 2;
    std::vector<double> trees(keep ? items * P : 0), rows(items * n * pffit::COLS);
    std::vector<int32_t> worst(items * n);
    std::vector<uint8_t> status(items);
    for (size_t item = 0; item < items; ++item) {
        std::unique_ptr<float[]> pred(new float[P]);
        std::unique_ptr<int32_t[]> sl(new int32_t[T]);
        std::unique_ptr<double[]> ln(new double[T]), tree(new double[P]), row(new double[n * pffit::COLS]);
        std::unique_ptr<int32_t[]> wj(new int32_t[n]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[1]);
        std::memcpy(pred.get(), preds.data() + item / (size_t)M * P, P * sizeof(float));
        std::memcpy(sl.get(), slots.data() + item * T, T * sizeof(int32_t));
        std::memcpy(ln.get(), lengths.data() + item * T, T * sizeof(double));
        pffit::run_serial(pred.get(), sl.get(), ln.get(), N, keep ? tree.get() : nullptr, row.get(), wj.get(), st.get());
        if (keep) std::memcpy(trees.data() + item * P, tree.get(), P * sizeof(double));
        std::memcpy(rows.data() + item * n * pffit::COLS, row.get(), n * pffit::COLS * sizeof(double));
        std::memcpy(worst.data() + item * n, wj.get(), n * sizeof(int32_t));
        status[item] = st[0];
    }
    FILE* out = std::fopen(argv[8], "wb");
    if (!out) { std::perror(argv[8]); return 2; }
    if (keep) std::fwrite(trees.data(), sizeof(double), trees.size(), out);
    std::fwrite(rows.data(), sizeof(double), rows.size(), out);
    std::fwrite(worst.data(), sizeof(int32_t), worst.size(), out);
    std::fwrite(status.data(), 1, status.size(), out);
    std::fclose(out);
    std::printf("clean, B = %d, M = %d, N = %d, keep = %d\n", B, M, N, keep);
    return 0;
}
