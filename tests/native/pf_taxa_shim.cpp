// Test-only C entry points over phyloformer_amd/csrc/pf_taxa_host.h (the taxon-table check of pf_forward_taxa and the
// pair-index rules of the leave-one-out reduction), for tests/test_taxa_host.py and, under AddressSanitizer / UBSan,
// tests/native/fuzz_taxa.py (compiled with g++; no HIP anywhere in this translation unit).
#include "../../phyloformer_amd/csrc/pf_taxa_host.h"

extern "C" {

long long t_first_bad_taxon(const int32_t* table, long long n, int N) { return pftaxa::first_bad_taxon(table, (size_t)n, N); }
long long t_pair_index(int i, int j, int N) { return pftaxa::pair_index(i, j, N); }
int t_pair_of(long long q, int N, int* i, int* j) { return pftaxa::pair_of(q, N, i, j) ? 1 : 0; }
long long t_loo_pair_index(int i, int j, int t, int N) { return pftaxa::loo_pair_index(i, j, t, N); }

}  // extern "C"
