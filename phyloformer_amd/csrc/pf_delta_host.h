// Delta scores (pf_delta, pf_delta_device, pf_delta_host): how far the quartets of a distance
// vector are from the four-point condition (Holland, Huber, Dress & Moulton 2002).  Plain C++, no HIP:
// tests/native/pf_delta_main.cpp runs the serial twin under AddressSanitizer / UBSan, pf_delta.hip.h compiles the
// quartet's arithmetic for the device too (PF_TAXA_HD).  phyloformer_amd/delta.py::delta_py is the statement: every
// float64 operation here happens with the same operands as there, and everything behind q is integer arithmetic, so
// the arrays are bit-identical whatever the order of the quartets.
//
// A quartet's three sums of two float32 distances widened to float64, one IEEE addition each; m1 >= m2 >= m3 by
// comparisons; delta = (m1 - m2) / (m1 - m3), 0 where m1 == m3; q = rint(delta 2^30), ties to even, in [0, 2^30].  The
// three sums enter symmetrically, so it does not matter which pairing of the four sequences is called s1.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pf_taxa_host.h"

namespace pfdelta {

constexpr int MIN_N = 4, MAX_N = 2048, MAX_K = 64;     // 3 C(N-1, 3) 2^30 < 2^63 up to N = 2,580
constexpr int Q_SHIFT = 30;

// NaN or infinite
PF_TAXA_HD inline bool nonfinite(float x) { return !(x - x == 0.0f); }

// index of the first pair of row i among the pairs of n sequences (i = n - 1: their number)
PF_TAXA_HD inline int64_t row_start(int64_t i, int64_t n) { return i * (2 * n - i - 1) / 2; }

// the pair (i, j), i < j, with index p: an estimate of the row by the square root, made exact by the integer test
PF_TAXA_HD inline void pair_of(int64_t p, int64_t n, int* i_out, int* j_out) {
    const double w = (double)(2 * n - 1);
    int64_t i = (int64_t)((w - sqrt(w * w - 8.0 * (double)p)) * 0.5);
    i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
    while (i < n - 2 && row_start(i + 1, n) <= p) ++i;
    while (i > 0 && row_start(i, n) > p) --i;
    *i_out = (int)i;
    *j_out = (int)(i + 1 + (p - row_start(i, n)));
}

// q of the sums s1, s2, s3 (finite)
PF_TAXA_HD inline int64_t quartet_q(double s1, double s2, double s3) {
    const double hi = s1 < s2 ? s2 : s1, lo = s1 < s2 ? s1 : s2;
    const double m1 = hi < s3 ? s3 : hi;
    const double m3 = s3 < lo ? s3 : lo;
    const double t = s3 < hi ? s3 : hi;                // min(max(s1, s2), s3)
    const double m2 = lo < t ? t : lo;
    const double den = m1 - m3;
    if (den == 0.0) return 0;
    const double delta = (m1 - m2) / den;
    return (int64_t)rint(delta * 1073741824.0);
}

// the bin of q among K
PF_TAXA_HD inline int bin_of(int64_t q, int K) {
    const int64_t b = (q * K) >> Q_SHIFT;
    return b < K - 1 ? (int)b : K - 1;
}

// what the three entry points refuse about (B, N, K): 0, or which of them (1: N, 2: B, 3: K)
inline int refused(int B, int N, int K) {
    if (N < MIN_N || N > MAX_N) return 1;
    if (B < 1) return 2;
    if (K < 1 || K > MAX_K) return 3;
    return 0;
}

// One source, every quartet a < b < c < d once: pair_sum [P_N], hist [K] (both zeroed here), the flag.
inline void run_serial(const float* preds, int N, int K, int64_t* pair_sum, int64_t* hist, uint8_t* flag) {
    const int64_t n = N, P = n * (n - 1) / 2;
    for (int64_t e = 0; e < P; ++e) pair_sum[e] = 0;
    for (int k = 0; k < K; ++k) hist[k] = 0;
    bool bad = false;
    for (int64_t e = 0; e < P; ++e) bad |= nonfinite(preds[e]);
    *flag = bad ? 1 : 0;
    if (bad) return;
    for (int64_t a = 0; a < n; ++a) {
        const int64_t ra = row_start(a, n) - a - 1;                      // pair (a, x) at ra + x
        for (int64_t b = a + 1; b < n; ++b) {
            const int64_t rb = row_start(b, n) - b - 1;
            const double dab = (double)preds[ra + b];
            for (int64_t c = b + 1; c < n; ++c) {
                const int64_t rc = row_start(c, n) - c - 1;
                const double dac = (double)preds[ra + c], dbc = (double)preds[rb + c];
                for (int64_t d = c + 1; d < n; ++d) {
                    const double s1 = dab + (double)preds[rc + d];
                    const double s2 = dac + (double)preds[rb + d];
                    const double s3 = (double)preds[ra + d] + dbc;
                    const int64_t q = quartet_q(s1, s2, s3);
                    pair_sum[ra + b] += q; pair_sum[ra + c] += q; pair_sum[ra + d] += q;
                    pair_sum[rb + c] += q; pair_sum[rb + d] += q; pair_sum[rc + d] += q;
                    ++hist[bin_of(q, K)];
                }
            }
        }
    }
}

// The arrays of a call as the caller or the staging of a host call holds them.
struct Tables { const float* preds; int64_t* pair_sum; int64_t* hist; uint8_t* flag; };
template <class V>
inline void staging_arrays(V& v, Tables& s, const Tables& u, size_t B, int N, int K) {
    const size_t P = (size_t)N * ((size_t)N - 1) / 2;
    v.out(s.pair_sum, u.pair_sum, B * P);
    v.out(s.hist, u.hist, B * (size_t)K);
    v.in(s.preds, u.preds, B * P);
    v.out(s.flag, u.flag, B);
}

}  // namespace pfdelta
