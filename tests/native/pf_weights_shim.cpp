// Test-only C entry points over phyloformer_amd/csrc/pf_weights_host.h (pattern compression, bootstrap counts, the
// padding rule and the weight check of the weighted entry points), so that tests/native/fuzz_weights.py can drive them
// under AddressSanitizer / UBSan (compiled with g++ -fsanitize=address,undefined; no HIP in this translation unit).
#include "../../phyloformer_amd/csrc/pf_weights_host.h"

extern "C" {

int t_padded_sites(int K, int L) { return pfweights::padded_sites(K, L); }
int t_boot_counts(int L, unsigned long long seed, int r, int32_t* sites, int32_t* counts) {
    return pfweights::boot_counts(L, seed, r, sites, counts);
}
long long t_compress_slots(int L) { return (long long)pfweights::compress_slots(L); }
int t_compress_sites(const uint8_t* idx, int N, int L, int32_t* first, int32_t* count, int32_t* slot) {
    return pfweights::compress_sites(idx, N, L, first, count, slot);
}
long long t_first_bad_weight(const float* w, long long n) { return pfweights::first_bad_weight(w, (size_t)n); }
float t_weight_sum(const float* w, int L) { return pfweights::weight_sum(w, L); }

}  // extern "C"
