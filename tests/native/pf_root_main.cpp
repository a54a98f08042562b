// The serial twin of the tree rooting (csrc/pf_root_host.h) as a stand-alone program for AddressSanitizer / UBSan
// (tests/test_root_host.py builds and runs it; nothing is loaded into Python).
//   pf_root_main B M N slots.bin lengths.bin result.bin
// slots.bin: int32 [B][M][T]; lengths.bin: float64 [B][M][T].  Every tree runs on exactly sized heap arrays of its own - the table
// too, so that a table that is none cannot be read past its end unnoticed.  result.bin: float64 ssq [B][M][T], pos [B][M][T], mid
// [B][M][5], uint8 status [B][M].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../phyloformer_amd/csrc/pf_root_host.h"

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
    if (argc != 7) { std::fprintf(stderr, "usage: pf_root_main B M N slots.bin lengths.bin result.bin\n"); return 2; }
    const int B = std::atoi(argv[1]), M = std::atoi(argv[2]), N = std::atoi(argv[3]);
    if (pfroot::refused(B, M, N)) { std::printf("refused %d\n", pfroot::refused(B, M, N)); return 3; }
    const size_t T = (size_t)pfroot::table_len(N), items = (size_t)B * (size_t)M, mid_len = (size_t)pfroot::MID;
    std::vector<int32_t> slots(items * T);
    std::vector<double> lengths(items * T);
    if (!read_all(argv[4], slots) || !read_all(argv[5], lengths)) return 2;
    std::vector<double> ssq(items * T), pos(items * T), mid(items * mid_len);
    std::vector<uint8_t> status(items);
    for (size_t item = 0; item < items; ++item) {
        std::unique_ptr<int32_t[]> sl(new int32_t[T]);
        std::unique_ptr<double[]> len(new double[T]), s(new double[T]), p(new double[T]), m(new double[mid_len]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[1]);
        std::memcpy(sl.get(), slots.data() + item * T, T * sizeof(int32_t));
        std::memcpy(len.get(), lengths.data() + item * T, T * sizeof(double));
        pfroot::run_serial(sl.get(), len.get(), N, s.get(), p.get(), m.get(), st.get());
        std::memcpy(ssq.data() + item * T, s.get(), T * sizeof(double));
        std::memcpy(pos.data() + item * T, p.get(), T * sizeof(double));
        std::memcpy(mid.data() + item * mid_len, m.get(), mid_len * sizeof(double));
        status[item] = st[0];
    }
    FILE* res = std::fopen(argv[6], "wb");
    if (!res) { std::perror(argv[6]); return 2; }
    std::fwrite(ssq.data(), sizeof(double), ssq.size(), res);
    std::fwrite(pos.data(), sizeof(double), pos.size(), res);
    std::fwrite(mid.data(), sizeof(double), mid.size(), res);
    std::fwrite(status.data(), 1, status.size(), res);
    std::fclose(res);
    std::printf("clean, B = %d, M = %d, N = %d\n", B, M, N);
    return 0;
}
