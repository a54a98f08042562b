// Host side of the site weights (pf_compress_sites, pf_boot_counts, pf_padded_sites, the weight check of
// pf_forward_weighted / pf_forward_sites_weighted).  Plain C++, no HIP: tests/native/pf_weights_shim.cpp drives it under
// AddressSanitizer / UBSan; phyloformer_amd/weights_sites.py holds the Python twins.
//
// An alignment in which site l occurs w_l times is the alignment of its distinct sites with every sum over sites
// weighted by w_l and L replaced by W = sum_l w_l.  What builds such tables:
//   compress_sites  the distinct columns of an alignment, in order of first occurrence, and how often each occurs;
//   boot_counts     the distinct sites of replicate r of the bootstrap stream (pf_boot.hip.h), ascending, and how often
//                   the replicate drew each;
//   padded_sites    the one shape a launch over tables of up to K entries takes: K rounded up to k_main's tile of 32
//                   tokens, never past L.  Padding entries are site 0 with weight 0.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace pfweights {

// min(L, 32 * ceil(K / 32)), or -1 for K < 1 or K > L
inline int padded_sites(int K, int L) {
    if (K < 1 || K > L) return -1;
    const int64_t up = ((int64_t)K + 31) / 32 * 32;
    return up < L ? (int)up : L;
}

// SplitMix64's finaliser: the bootstrap stream's mixer (pf_boot.hip.h::mix64, bootstrap.py::mix64)
inline uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// Replicate r of the stream of `seed` over L sites: sites[0..K) its distinct source sites, ascending, counts[0..K) how
// often it drew each (they sum to L).  Both buffers hold L entries: counts is the histogram while the draws run and is
// compacted in place (entry j is written only after entry s >= j was read).  Returns K, or -1 for L < 1 or r < 0.
inline int boot_counts(int L, uint64_t seed, int r, int32_t* sites, int32_t* counts) {
    if (L < 1 || r < 0) return -1;
    const uint64_t key = mix64(seed + 0x9E3779B97F4A7C15ull), hi = (uint64_t)(uint32_t)r << 32;
    memset(counts, 0, (size_t)L * sizeof(int32_t));
    for (int l = 0; l < L; ++l) {
        const uint64_t z = mix64(key ^ (hi | (uint32_t)l));
        ++counts[(size_t)(((z >> 32) * (uint64_t)(uint32_t)L) >> 32)];
    }
    int K = 0;
    for (int s = 0; s < L; ++s) {
        const int32_t c = counts[s];
        if (c) { sites[K] = s; counts[K] = c; ++K; }
    }
    return K;
}

// The distinct columns of idx [N][L] in order of first occurrence: first[k] the site where column k first stands,
// count[k] how often it occurs (they sum to L).  first and count hold L entries; the scratch `slot` holds
// compress_slots(L) - a power of two >= 2 L: an open-addressing table of column numbers keyed by an FNV-1a hash of the
// column's bytes; equal hashes are told apart by comparing the columns.  Returns K, or -1 for N < 1 or L < 1.
inline size_t compress_slots(int L) {
    size_t n = 16;
    while (n < 2 * (size_t)(L > 0 ? L : 0)) n <<= 1;
    return n;
}
inline int compress_sites(const uint8_t* idx, int N, int L, int32_t* first, int32_t* count, int32_t* slot /* [compress_slots(L)] */) {
    if (N < 1 || L < 1) return -1;
    const size_t cap = compress_slots(L), mask = cap - 1;
    for (size_t i = 0; i < cap; ++i) slot[i] = -1;
    int K = 0;
    for (int l = 0; l < L; ++l) {
        uint64_t hsh = 0xCBF29CE484222325ull;
        for (int n = 0; n < N; ++n) hsh = (hsh ^ idx[(size_t)n * L + l]) * 0x100000001B3ull;
        size_t at = (size_t)mix64(hsh) & mask;
        for (;; at = (at + 1) & mask) {
            const int32_t k = slot[at];
            if (k < 0) { slot[at] = K; first[K] = l; count[K] = 1; ++K; break; }
            const int f = first[k];
            bool same = true;
            for (int n = 0; n < N && same; ++n) same = idx[(size_t)n * L + f] == idx[(size_t)n * L + l];
            if (same) { ++count[k]; break; }
        }
    }
    return K;
}

// index of the first entry of w[n] that is negative or not finite (NaN included), or -1: one branch-free pass, the
// offender is looked for only if there is one
inline int64_t first_bad_weight(const float* w, size_t n) {
    unsigned bad = 0;
    for (size_t i = 0; i < n; ++i) bad |= (unsigned)!(w[i] >= 0.f && w[i] <= 3.402823466e38f);
    if (bad)
        for (size_t i = 0; i < n; ++i)
            if (!(w[i] >= 0.f && w[i] <= 3.402823466e38f)) return (int64_t)i;
    return -1;
}

// W of one alignment: its weights added in site order, in float - the order and format of k_weight_sums
// (pf_weights.hip.h), which computes the W the kernels use; the host sum only decides the refusal of W == 0 / inf
inline float weight_sum(const float* w, int L) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += w[l];
    return s;
}

}  // namespace pfweights
