// Test-only C entry points over phyloformer_amd/csrc/pf_sites_host.h (the window rule and the site-table check of
// pf_forward_windows / pf_forward_sites), so that tests/native/fuzz_sites.py can drive them under AddressSanitizer /
// UBSan (compiled with g++ -fsanitize=address,undefined; no HIP anywhere in this translation unit).
#include "../../phyloformer_amd/csrc/pf_sites_host.h"

extern "C" {

int t_window_count(int L, int W, int step) { return pfsites::window_count(L, W, step); }
int t_window_start(int L, int W, int step, int s) { return pfsites::window_start(L, W, step, s); }
long long t_first_bad_site(const int32_t* sites, long long n, int L) { return pfsites::first_bad_site(sites, (size_t)n, L); }

}  // extern "C"
