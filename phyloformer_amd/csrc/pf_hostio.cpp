// Host-side file-format helpers of the inference CLI (no GPU work, no HIP calls).
//
// The reference does both in per-element Python loops:
//   - FASTA -> one-hot   phyloformer/data.py:11-31   (here: bytes -> uint8 residue indices [N][L])
//   - distances -> PHYLIP text   infer_alns.py:14-25   (here: float [P] -> "%.10f" square matrix)
// At 60 x 500 those loops cost ~3 ms per alignment in CPython, more than the MI355X forward pass
// (2.3 ms), and hold the GIL.  These two functions do the same work in ~0.2 ms and are called through
// ctypes (GIL released), so the CLI's loader / writer threads scale with host cores.
#include <algorithm>
#include <atomic>
#include <charconv>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/phyloformer_amd.h"
#include "pf_bme_host.h"
#include "pf_bionj_host.h"
#include "pf_delta_host.h"
#include "pf_fit_host.h"
#include "pf_ols_host.h"
#include "pf_root_host.h"
#include "pf_support_host.h"
#include "pf_consensus_host.h"
#include "pf_treedist_host.h"

namespace {

const char kAlphabet[] = "ARNDCQEGHILKMFPSTWYVX-";   // phyloformer/data.py:7

struct Lut {
    uint8_t v[256];
    Lut() {
        memset(v, 255, sizeof v);
        for (int i = 0; kAlphabet[i]; ++i) v[(unsigned char)kAlphabet[i]] = (uint8_t)i;
    }
};
const Lut kLut;

// "%.10f" of a float, exactly as printf / CPython format it (round-half-even on the exact binary value),
// without printf's arbitrary-precision machinery: a float is m * 2^e with m < 2^24, so m * 10^10 < 2^58
// fits an integer and the rounding is one shift and one comparison.
inline int format_f10(float x, char* out) {
    uint32_t bits;
    memcpy(&bits, &x, 4);
    int w = 0;
    const uint32_t ex = (bits >> 23) & 0xff;
    uint64_t m = bits & 0x7fffffu;
    if (ex == 0xff) {
        if (m) { memcpy(out, "nan", 3); return 3; }
        if (bits >> 31) out[w++] = '-';
        memcpy(out + w, "inf", 3);
        return w + 3;
    }
    if (bits >> 31) out[w++] = '-';
    int e;                                   // value = m * 2^e
    if (ex == 0) e = -149; else { m |= 0x800000u; e = (int)ex - 150; }
    unsigned __int128 q;                     // round(value * 10^10)
    if (e >= 0) {
        if (e > 60)                          // > 2^84: far outside any distance; let printf do it
            return w + snprintf(out + w, 64, "%.10f", (double)(x < 0 ? -x : x));
        q = ((unsigned __int128)m << e) * 10000000000ull;   // < 2^(24 + 60 + 34)
    } else {
        const unsigned __int128 n = (unsigned __int128)m * 10000000000ull;
        const int s = -e;
        if (s >= 100) q = 0;                 // n < 2^58 < half an ulp of the last printed digit
        else {
            q = n >> s;
            const unsigned __int128 rem = n - (q << s), half = (unsigned __int128)1 << (s - 1);
            if (rem > half || (rem == half && (q & 1))) ++q;
        }
    }
    const unsigned __int128 ten10 = 10000000000ull;
    unsigned __int128 ip = q / ten10;
    uint64_t fp = (uint64_t)(q % ten10);
    char tmp[48];
    int k = 0;
    do { tmp[k++] = (char)('0' + (int)(ip % 10)); ip /= 10; } while (ip);
    while (k) out[w++] = tmp[--k];
    out[w++] = '.';
    for (int i = 9; i >= 0; --i) { out[w + i] = (char)('0' + fp % 10); fp /= 10; }
    return w + 10;
}

// bytes.strip() of CPython: space, \t, \n, \r, \x0b, \x0c
inline bool is_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }

// Would bytes.decode("utf8") accept [p, p + n)?  (CPython's strict decoder: no overlong forms, no surrogates,
// nothing above U+10FFFF.)  The reference decodes every header where it meets it (data.py:22).
inline bool valid_utf8(const unsigned char* p, int64_t n) {
    int64_t i = 0;
    while (i < n) {
        const unsigned char c = p[i];
        if (c < 0x80) { ++i; continue; }
        int extra;
        unsigned char lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) extra = 1;
        else if (c == 0xE0) { extra = 2; lo = 0xA0; }
        else if (c >= 0xE1 && c <= 0xEC) extra = 2;
        else if (c == 0xED) { extra = 2; hi = 0x9F; }
        else if (c >= 0xEE && c <= 0xEF) extra = 2;
        else if (c == 0xF0) { extra = 3; lo = 0x90; }
        else if (c >= 0xF1 && c <= 0xF3) extra = 3;
        else if (c == 0xF4) { extra = 3; hi = 0x8F; }
        else return false;
        if (i + extra >= n) return false;                  // truncated sequence
        if (p[i + 1] < lo || p[i + 1] > hi) return false;
        for (int k = 2; k <= extra; ++k)
            if (p[i + k] < 0x80 || p[i + k] > 0xBF) return false;
        i += extra + 1;
    }
    return true;
}

}  // namespace

extern "C" {

int pf_parse_fasta(const char* data, int64_t len, uint8_t* idx, int64_t idx_cap, int64_t* id_spans,
                   int32_t max_seqs, int32_t* n_out, int32_t* l_out, int64_t* detail) {
    if (!data || len < 0 || !n_out || !l_out) return PF_EINVAL;
    int64_t dummy = 0;
    if (!detail) detail = &dummy;
    *detail = 0;
    int32_t n = 0;
    int64_t cur_len = 0;      // residues of the current record
    int64_t first_len = -1;   // residues of record 0
    int64_t written = 0;
    bool ragged = false;
    int64_t pos = 0;
    while (pos <= len) {
        // one line: [pos, eol), split on '\n' only (binary file iteration)
        const char* nl = pos < len ? (const char*)memchr(data + pos, '\n', (size_t)(len - pos)) : nullptr;
        int64_t eol = nl ? (int64_t)(nl - data) : len;
        int64_t a = pos, b = eol;
        while (a < b && is_space((unsigned char)data[a])) ++a;
        while (b > a && is_space((unsigned char)data[b - 1])) --b;
        if (a < b) {
            if (data[a] == '>') {
                if (n > 0) {
                    if (first_len < 0) first_len = cur_len;
                    else if (cur_len != first_len) ragged = true;
                }
                if (!valid_utf8((const unsigned char*)data + a + 1, b - (a + 1))) {
                    *detail = a + 1;                     // offset of the id: the caller decodes it to raise
                    *n_out = n;
                    return PF_FASTA_EUTF8;
                }
                if (id_spans) {
                    if (n >= max_seqs) return PF_FASTA_ECAP;
                    id_spans[2 * n] = a + 1;
                    id_spans[2 * n + 1] = b - (a + 1);
                }
                ++n;
                cur_len = 0;
            } else {
                if (n == 0) return PF_FASTA_ENOHEADER;
                for (int64_t i = a; i < b; ++i) {
                    uint8_t r = kLut.v[(unsigned char)data[i]];
                    if (r == 255) { *detail = (unsigned char)data[i]; return PF_FASTA_EBYTE; }
                    if (idx) {
                        if (written >= idx_cap) return PF_FASTA_ECAP;
                        idx[written] = r;
                    }
                    ++written;
                }
                cur_len += b - a;
            }
        }
        if (!nl) break;
        pos = eol + 1;
    }
    if (n == 0) return PF_FASTA_EEMPTY;
    if (first_len < 0) first_len = cur_len;
    else if (cur_len != first_len) ragged = true;
    *n_out = n;
    if (ragged) { *l_out = -1; return PF_FASTA_ERAGGED; }
    *l_out = (int32_t)first_len;
    return PF_OK;
}

// ids[i] has id_lens[i] bytes (id_lens == NULL: NUL-terminated)
static int64_t format_phylip_impl(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens,
                                  char* out, int64_t cap) {
    if (!preds || n < 1 || !ids || (!out && cap > 0)) return PF_EINVAL;
    int64_t w = 0;
    char num[96];
    auto put = [&](const char* s, int64_t k) {
        if (out && w + k <= cap) memcpy(out + w, s, (size_t)k);
        w += k;
    };
    int k = snprintf(num, sizeof num, "%d\n", n);
    put(num, k);
    // pair (i, j), i < j, lexicographic: offset of row i is i*n - i*(i+1)/2 - (i+1)
    auto at = [&](int64_t i, int64_t j) -> float {
        if (i == j) return 0.0f;
        if (i > j) { int64_t t = i; i = j; j = t; }
        // dm + dm.T of the reference (infer_alns.py:19-20) adds the zero of the other triangle: -0.0 becomes 0.0
        return preds[i * n - i * (i + 1) / 2 + (j - i - 1)] + 0.0f;
    };
    for (int32_t i = 0; i < n; ++i) {
        const char* id = ids[i] ? ids[i] : "";
        put(id, id_lens ? id_lens[i] : (int64_t)strlen(id));
        put(" ", 1);
        for (int32_t j = 0; j < n; ++j) {
            if (j) put(" ", 1);
            k = format_f10(at(i, j), num);
            put(num, k);
        }
        put("\n", 1);
    }
    return w;
}

int64_t pf_format_phylip(const float* preds, int32_t n, const char* const* ids, char* out, int64_t cap) {
    return format_phylip_impl(preds, n, ids, nullptr, out, cap);
}
int64_t pf_format_phylip_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, char* out,
                           int64_t cap) {
    if (!id_lens) return PF_EINVAL;
    for (int32_t i = 0; i < n; ++i) if (id_lens[i] < 0) return PF_EINVAL;
    return format_phylip_impl(preds, n, ids, id_lens, out, cap);
}

}  // extern "C"

// ---- neighbour joining + Newick text (the CLI's --trees: infer_alns.py:62-64,120-123) -------------------------------
//
// The reference calls skbio.tree.nj (not installed here); phyloformer_amd/nj.py is this build's pinned statement of
// the algorithm (FastME -m N goldens, tests/test_treecmp.py) and THIS function is its native twin: the same float64
// operations in the same order - numpy's pairwise row sums included - and Python's repr() of the branch lengths, so
// that the .nj.nwk files are byte-identical to nj.py's (tests/test_host.py) while `-t` stays on the native file
// pipeline (with `-t` every file used to fall back to per-file Python under the GIL).
namespace {

// numpy's add.reduce over a contiguous row (DOUBLE_pairwise_sum): < 8 sequential, <= 128 eight accumulators, else halves
double np_pairwise_sum(const double* a, int64_t n) {
    if (n < 8) {
        double res = -0.0;
        for (int64_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// Python's repr(float): the shortest digits that round-trip, fixed notation for -4 < decimal point <= 16 (with ".0" for
// integers), else d.ddde+XX with at least two exponent digits
void append_repr(std::string& out, double x) {
    if (x != x) { out += "nan"; return; }
    if (x == INFINITY || x == -INFINITY) { out += x < 0 ? "-inf" : "inf"; return; }
    char buf[64];
    const auto r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::scientific);   // [-]d[.ddd]e[+-]XX, shortest
    const char* p = buf;
    if (*p == '-') { out += '-'; ++p; }
    char digits[32];
    int nd = 0;
    for (; p < r.ptr && *p != 'e'; ++p)
        if (*p != '.') digits[nd++] = *p;
    int e10 = 0;
    if (p < r.ptr && *p == 'e') {
        ++p;
        const bool neg = *p == '-';
        if (*p == '-' || *p == '+') ++p;
        for (; p < r.ptr; ++p) e10 = e10 * 10 + (*p - '0');
        if (neg) e10 = -e10;
    }
    const int decpt = e10 + 1;
    if (-4 < decpt && decpt <= 16) {
        if (decpt <= 0) {
            out += "0.";
            out.append((size_t)(-decpt), '0');
            out.append(digits, (size_t)nd);
        } else if (decpt >= nd) {
            out.append(digits, (size_t)nd);
            out.append((size_t)(decpt - nd), '0');
            out += ".0";
        } else {
            out.append(digits, (size_t)decpt);
            out += '.';
            out.append(digits + decpt, (size_t)(nd - decpt));
        }
    } else {
        out += digits[0];
        if (nd > 1) { out += '.'; out.append(digits + 1, (size_t)(nd - 1)); }
        char ex[16];
        const int e = decpt - 1;
        snprintf(ex, sizeof ex, "e%c%02d", e < 0 ? '-' : '+', e < 0 ? -e : e);
        out += ex;
    }
}

// preds [n(n-1)/2] (pairs i < j, lexicographic): the symmetric matrix vec_to_phylip builds (float32, dm + dm.T)
double pair_at(const float* preds, int64_t n, int64_t i, int64_t j) {
    if (i == j) return 0.0;
    if (i > j) { const int64_t t = i; i = j; j = t; }
    return (double)(preds[i * n - i * (i + 1) / 2 + (j - i - 1)] + 0.0f);
}

// The join sequence of neighbour joining (nj.py::nj_joins): join t merges slots a < b into slot a; the last three
// slots meet at the trifurcation.
struct NjJoin { int32_t a, b; double la, lb; };
struct NjTree {
    std::vector<NjJoin> joins;
    int32_t i = 0, j = 0, k = 0;
    double li = 0, lj = 0, lk = 0;
};

// The join table of a tree (pf_nj_joins: slots / lengths [pfnj::table_len(n)], n >= 3: the joins a, b / la, lb, then the
// trifurcation i, j, k / li, lj, lk) and back: the two places that know the layout
NjTree tree_of_table(const int32_t* slots, const double* lengths, int32_t n) {
    const size_t joins = (size_t)n - 3;
    NjTree t;
    t.joins.reserve(joins);
    for (size_t s = 0; s < joins; ++s) t.joins.push_back({slots[2 * s], slots[2 * s + 1], lengths[2 * s], lengths[2 * s + 1]});
    slots += 2 * joins; lengths += 2 * joins;
    t.i = slots[0]; t.j = slots[1]; t.k = slots[2];
    t.li = lengths[0]; t.lj = lengths[1]; t.lk = lengths[2];
    return t;
}

void table_of_tree(const NjTree& t, int32_t* slots, double* lengths) {
    for (const NjJoin& jn : t.joins) { *slots++ = jn.a; *slots++ = jn.b; *lengths++ = jn.la; *lengths++ = jn.lb; }
    slots[0] = t.i; slots[1] = t.j; slots[2] = t.k;
    lengths[0] = t.li; lengths[1] = t.lj; lengths[2] = t.lk;
}

// ids[i] has id_lens[i] bytes (id_lens == NULL: NUL-terminated)
std::string label_of(const char* const* ids, const int64_t* id_lens, int32_t i) {
    const char* id = ids[i] ? ids[i] : "";
    return std::string(id, (size_t)(id_lens ? id_lens[i] : (int64_t)strlen(id)));
}

// The frame of a text entry point: what every such call refuses, then `fill` (text -> PF_OK or the code to return)
// under the catch-all, the text copied out where it fits `cap`, and its size - the sizing protocol of pf_format_phylip.
// What a call refuses beyond this stands at the call: before this where it is tested before the id lengths, in `fill`
// where after.
template <class Fill>
int64_t text_call(int32_t n, const char* const* ids, const int64_t* id_lens, char* out, int64_t cap, Fill&& fill) {
    if (n < 1 || !ids || !id_lens || (!out && cap > 0)) return PF_EINVAL;
    for (int32_t i = 0; i < n; ++i) if (id_lens[i] < 0) return PF_EINVAL;
    try {
        std::string text;
        const int rc = fill(text);
        if (rc != PF_OK) return rc;
        if (out && (int64_t)text.size() <= cap) memcpy(out, text.data(), text.size());
        return (int64_t)text.size();
    } catch (...) { return PF_ENOMEM; }
}

// n >= 3
void nj_core(const float* preds, int32_t n, NjTree& t) {
    const size_t N = (size_t)n;
    std::vector<double> d(N * N), sub, r, dn(N);
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j < N; ++j) d[i * N + j] = pair_at(preds, n, (int64_t)i, (int64_t)j);
    std::vector<int32_t> active((size_t)n);
    for (int32_t i = 0; i < n; ++i) active[(size_t)i] = i;
    t.joins.clear();
    t.joins.reserve(N - 3);
    while (active.size() > 3) {
        const size_t m = active.size();
        sub.resize(m * m);
        r.resize(m);
        for (size_t a = 0; a < m; ++a)
            for (size_t b = 0; b < m; ++b) sub[a * m + b] = d[(size_t)active[a] * N + (size_t)active[b]];
        for (size_t a = 0; a < m; ++a) r[a] = np_pairwise_sum(&sub[a * m], (int64_t)m);
        // q = (m - 2) * sub - r[:, None] - r[None, :], diagonal = inf; the first minimum in row-major order (np.argmin)
        const double mm2 = (double)((int64_t)m - 2);
        double best = INFINITY;
        size_t ba = 0, bb = 0;
        bool have = false, saw_nan = false;
        for (size_t a = 0; a < m && !saw_nan; ++a)
            for (size_t b = 0; b < m; ++b) {
                const double q = a == b ? INFINITY : (mm2 * sub[a * m + b] - r[a]) - r[b];
                if (q != q) { ba = a; bb = b; saw_nan = true; have = true; break; }     // np.argmin: the first NaN wins
                if (!have || q < best) { best = q; ba = a; bb = b; have = true; }
            }
        if (ba > bb) { const size_t tmp = ba; ba = bb; bb = tmp; }
        const size_t ia = (size_t)active[ba], ib = (size_t)active[bb];
        const double dab = sub[ba * m + bb];
        const double la = 0.5 * dab + (r[ba] - r[bb]) / (double)(2 * ((int64_t)m - 2));
        const double lb = dab - la;
        t.joins.push_back({(int32_t)ia, (int32_t)ib, la, lb});
        for (size_t k = 0; k < N; ++k) dn[k] = 0.5 * ((d[ia * N + k] + d[ib * N + k]) - dab);
        for (size_t k = 0; k < N; ++k) { d[ia * N + k] = dn[k]; d[k * N + ia] = dn[k]; }
        d[ia * N + ia] = 0.0;
        active.erase(active.begin() + (std::ptrdiff_t)bb);
    }
    const size_t i = (size_t)active[0], j = (size_t)active[1], k = (size_t)active[2];
    t.i = (int32_t)i; t.j = (int32_t)j; t.k = (int32_t)k;
    t.li = 0.5 * ((d[i * N + j] + d[i * N + k]) - d[j * N + k]);
    t.lj = 0.5 * ((d[i * N + j] + d[j * N + k]) - d[i * N + k]);
    t.lk = 0.5 * ((d[i * N + k] + d[j * N + k]) - d[i * N + j]);
}

// Newick text of a join sequence (nj.py::newick_of_joins); support[t], when not NULL, follows the ')' of join t's node
void nj_format(const NjTree& t, int32_t n, const char* const* ids, const int64_t* id_lens, bool clamp,
               const int32_t* support, std::string& out) {
    std::vector<std::string> labels((size_t)n);
    for (int32_t i = 0; i < n; ++i) labels[(size_t)i] = label_of(ids, id_lens, i);
    auto fmt = [&](std::string& dst, double x) {
        if (clamp && x < 0) x = 0.0;
        append_repr(dst, x);
    };
    for (size_t s = 0; s < t.joins.size(); ++s) {
        const NjJoin& jn = t.joins[s];
        const size_t ia = (size_t)jn.a, ib = (size_t)jn.b;
        std::string nl;
        nl.reserve(labels[ia].size() + labels[ib].size() + 64);
        nl += '('; nl += labels[ia]; nl += ':'; fmt(nl, jn.la); nl += ','; nl += labels[ib]; nl += ':'; fmt(nl, jn.lb); nl += ')';
        if (support) nl += std::to_string(support[s]);
        labels[ia].swap(nl);
        std::string().swap(labels[ib]);
    }
    const size_t i = (size_t)t.i, j = (size_t)t.j, k = (size_t)t.k;
    out.clear();
    out.reserve(labels[i].size() + labels[j].size() + labels[k].size() + 96);
    out += '('; out += labels[i]; out += ':'; fmt(out, t.li); out += ','; out += labels[j]; out += ':'; fmt(out, t.lj);
    out += ','; out += labels[k]; out += ':'; fmt(out, t.lk); out += ");\n";
}

// preds [n(n-1)/2] -> Newick text of the neighbour-joining tree, as nj.py::neighbor_joining writes it
void nj_newick(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, bool clamp, std::string& out) {
    out.clear();
    auto label = [&](int32_t i) { return label_of(ids, id_lens, i); };
    if (n == 1) { out = "(" + label(0) + ");\n"; return; }
    if (n == 2) {
        char num[64];
        snprintf(num, sizeof num, "%.6g", pair_at(preds, n, 0, 1) / 2);
        out = "(" + label(0) + ":" + num + "," + label(1) + ":" + num + ");\n";
        return;
    }
    NjTree t;
    nj_core(preds, n, t);
    nj_format(t, n, ids, id_lens, clamp, nullptr, out);
}

// The split each join creates: a bitset over sequence indices (W words each), normalised to the side without
// sequence 0 (bootstrap.py::join_splits).  splits [joins][W]
void nj_splits(const NjTree& t, int32_t n, std::vector<uint64_t>& splits) {
    const size_t W = ((size_t)n + 63) / 64;
    std::vector<uint64_t> members((size_t)n * W, 0);
    for (int32_t i = 0; i < n; ++i) members[(size_t)i * W + (size_t)i / 64] = 1ull << (i % 64);
    splits.assign(t.joins.size() * W, 0);
    for (size_t s = 0; s < t.joins.size(); ++s) {
        uint64_t* ma = &members[(size_t)t.joins[s].a * W];
        const uint64_t* mb = &members[(size_t)t.joins[s].b * W];
        for (size_t w = 0; w < W; ++w) ma[w] |= mb[w];
        const bool flip = ma[0] & 1u;
        for (size_t w = 0; w < W; ++w) {
            const int bits = (int)std::min<size_t>(64, (size_t)n - 64 * w);
            const uint64_t mask = bits == 64 ? ~0ull : ((1ull << bits) - 1);
            splits[s * W + w] = flip ? (~ma[w] & mask) : ma[w];
        }
    }
}

}  // namespace

extern "C" {

int64_t pf_nj_newick_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                       char* out, int64_t cap) {
    if (!preds) return PF_EINVAL;
    return text_call(n, ids, id_lens, out, cap, [&](std::string& text) {
        nj_newick(preds, n, ids, id_lens, clamp_negative != 0, text);
        return PF_OK;
    });
}

// The Newick text of a join table (pf_nj_joins: slots / lengths [2 (n - 3) + 3], n >= 3) through nj_format: the text
// of nj.py::newick_of_joins, and of pf_nj_newick_n for the table of the same distances.  PF_EINVAL also for a slot
// outside [0, n).
int64_t pf_nj_format_joins_n(const int32_t* slots, const double* lengths, int32_t n, const char* const* ids, const int64_t* id_lens,
                             int32_t clamp_negative, char* out, int64_t cap) {
    if (!slots || !lengths || n < 3) return PF_EINVAL;
    return text_call(n, ids, id_lens, out, cap, [&](std::string& text) {
        for (int64_t k = 0; k < pfnj::table_len(n); ++k) if (slots[k] < 0 || slots[k] >= n) return PF_EINVAL;
        nj_format(tree_of_table(slots, lengths, n), n, ids, id_lens, clamp_negative != 0, nullptr, text);
        return PF_OK;
    });
}

}  // extern "C"

extern "C" {

// ---- many files per call, on native threads (no GIL anywhere near the file system) ---------------------------
//
// The CLI's loop over a directory (infer_alns.py:97-117) opens, parses and writes one small file per
// alignment; at 20 x 200 the MI355X finishes 11,000 alignments a second, and CPython - one open() / read() /
// parse / format / write() per file under the GIL - delivered 6,000.  These entry points take a
// LIST of paths: a pool of std::threads reads and parses (or formats and writes) them, the results stay in a
// library-owned batch object that the writer later takes the sequence ids from, so Python touches neither
// the residues nor the ids of an alignment on the fast path.

}  // extern "C"

struct pf_fasta_batch {
    struct File {
        int32_t status = PF_EINVAL, n = 0, l = 0;
        int64_t detail = 0;
        std::vector<uint8_t> idx;          // [n][l]
        std::string ids;                   // the ids back to back
        std::vector<int64_t> spans;        // (offset, length) per id, into `ids`
    };
    std::vector<File> files;
};

namespace {

template <typename F>
void run_pool(int32_t count, int32_t threads, F&& fn) {
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads, count));
    if (nt == 1) { for (int32_t i = 0; i < count; ++i) { try { fn(i); } catch (...) {} } return; }
    std::atomic<int32_t> next{0};
    // (an exception that escaped a std::thread body would be std::terminate: the callers' lambdas record failures per
    // item, and whatever they did not foresee ends here - ADVICE r05)
    auto work = [&] { for (int32_t i = next.fetch_add(1); i < count; i = next.fetch_add(1)) { try { fn(i); } catch (...) {} } };
    std::vector<std::thread> pool;
    pool.reserve(nt);
    // the calling thread is one of the workers; a thread the system refuses to start (EAGAIN) only narrows the pool -
    // nothing may throw across the C ABI
    for (int t = 1; t < nt; ++t) {
        try { pool.emplace_back(work); } catch (...) { break; }
    }
    work();
    for (auto& th : pool) th.join();
}

// whole file -> buf; 0 or -errno
int read_file(const char* path, std::string& buf) {
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return -errno;
    struct stat st;
    if (fstat(fd, &st) != 0) { const int e = errno; close(fd); return -e; }
    if (S_ISDIR(st.st_mode)) { close(fd); return -EISDIR; }
    buf.resize(st.st_size > 0 ? (size_t)st.st_size : 0);
    size_t got = 0;
    for (;;) {
        if (got == buf.size()) buf.resize(buf.size() ? buf.size() * 2 : 65536);      // grew, or size unknown
        const ssize_t r = read(fd, &buf[got], buf.size() - got);
        if (r < 0) { if (errno == EINTR) continue; const int e = errno; close(fd); return -e; }
        if (r == 0) break;
        got += (size_t)r;
        if (got == (size_t)st.st_size && st.st_size > 0) {                           // the common case: one read
            char probe;
            const ssize_t more = read(fd, &probe, 1);
            if (more <= 0) break;
            buf.push_back(probe);
            got += 1;
        }
    }
    close(fd);
    buf.resize(got);
    return 0;
}

void load_one(const char* path, pf_fasta_batch::File& f) {
    std::string data;
    const int rc = read_file(path, data);
    if (rc) { f.status = PF_EIO; f.detail = -rc; return; }
    int64_t nrec = 1;
    for (char c : data) nrec += (c == '>');
    f.idx.resize(data.size() ? data.size() : 1);
    std::vector<int64_t> spans((size_t)2 * nrec);
    f.status = pf_parse_fasta(data.data(), (int64_t)data.size(), f.idx.data(), (int64_t)f.idx.size(), spans.data(),
                              (int32_t)std::min<int64_t>(nrec, INT32_MAX), &f.n, &f.l, &f.detail);
    if (f.status != PF_OK) { f.idx.clear(); f.idx.shrink_to_fit(); return; }
    f.idx.resize((size_t)f.n * (size_t)f.l);
    f.idx.shrink_to_fit();
    f.spans.resize((size_t)2 * f.n);
    for (int32_t i = 0; i < f.n; ++i) {
        f.spans[2 * i] = (int64_t)f.ids.size();
        f.spans[2 * i + 1] = spans[2 * i + 1];
        f.ids.append(data.data() + spans[2 * i], (size_t)spans[2 * i + 1]);
    }
}

// 0 or -errno
int write_file(const char* path, const char* data, size_t len) {
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) return -errno;
    size_t done = 0;
    while (done < len) {
        const ssize_t r = write(fd, data + done, len - done);
        if (r < 0) { if (errno == EINTR) continue; const int e = errno; close(fd); return -e; }
        done += (size_t)r;
    }
    return close(fd) == 0 ? 0 : -errno;
}

}  // namespace

extern "C" {

int pf_fasta_batch_load(const char* const* paths, int32_t count, int32_t threads, pf_fasta_batch_t** out) {
    if (!paths || count < 0 || !out) return PF_EINVAL;
    for (int32_t i = 0; i < count; ++i) if (!paths[i]) return PF_EINVAL;
    pf_fasta_batch* b = new (std::nothrow) pf_fasta_batch();
    if (!b) return PF_ENOMEM;
    try {
        b->files.resize((size_t)count);
        run_pool(count, threads, [&](int32_t i) {
            try { load_one(paths[i], b->files[(size_t)i]); }
            catch (const std::bad_alloc&) { b->files[(size_t)i].status = PF_ENOMEM; }
        });
    } catch (...) { delete b; return PF_ENOMEM; }
    *out = b;
    return PF_OK;
}

void pf_fasta_batch_free(pf_fasta_batch_t* b) { delete b; }

int32_t pf_fasta_batch_count(const pf_fasta_batch_t* b) { return b ? (int32_t)b->files.size() : 0; }

int pf_fasta_batch_infos(const pf_fasta_batch_t* b, int32_t* status, int32_t* n, int32_t* l, int64_t* detail) {
    if (!b || !status || !n || !l || !detail) return PF_EINVAL;
    for (size_t i = 0; i < b->files.size(); ++i) {
        const auto& f = b->files[i];
        status[i] = f.status; n[i] = f.n; l[i] = f.l; detail[i] = f.detail;
    }
    return PF_OK;
}

int pf_fasta_batch_id(const pf_fasta_batch_t* b, int32_t file, int32_t seq, const char** id, int64_t* len) {
    if (!b || !id || !len || file < 0 || (size_t)file >= b->files.size()) return PF_EINVAL;
    const auto& f = b->files[(size_t)file];
    if (f.status != PF_OK || seq < 0 || seq >= f.n) return PF_EINVAL;
    *id = f.ids.data() + f.spans[2 * (size_t)seq];
    *len = f.spans[2 * (size_t)seq + 1];
    return PF_OK;
}

int pf_fasta_batch_gather(const pf_fasta_batch_t* const* batches, const int32_t* file_idx, int32_t count, int32_t n,
                          int32_t l, uint8_t* dst) {
    if (!batches || !file_idx || count < 0 || n < 1 || l < 0 || !dst) return PF_EINVAL;
    const size_t per = (size_t)n * (size_t)l;
    for (int32_t k = 0; k < count; ++k) {
        const pf_fasta_batch* b = batches[k];
        if (!b || file_idx[k] < 0 || (size_t)file_idx[k] >= b->files.size()) return PF_EINVAL;
        const auto& f = b->files[(size_t)file_idx[k]];
        if (f.status != PF_OK || f.n != n || f.l != l || f.idx.size() != per) return PF_EINVAL;
        if (per) memcpy(dst + (size_t)k * per, f.idx.data(), per);
    }
    return PF_OK;
}

int pf_phylip_write_batch(const pf_fasta_batch_t* const* batches, const int32_t* file_idx, int32_t count, int32_t n,
                          const float* preds, const char* const* out_paths, const char* const* tree_paths, int32_t threads,
                          int32_t* status) {
    if (!batches || !file_idx || count < 0 || n < 2 || !preds || !out_paths || !status) return PF_EINVAL;
    for (int32_t k = 0; k < count; ++k) {
        const pf_fasta_batch* b = batches[k];
        if (!b || !out_paths[k] || (tree_paths && !tree_paths[k]) || file_idx[k] < 0 || (size_t)file_idx[k] >= b->files.size())
            return PF_EINVAL;
        const auto& f = b->files[(size_t)file_idx[k]];
        if (f.status != PF_OK || f.n != n) return PF_EINVAL;
    }
    const size_t P = (size_t)n * (size_t)(n - 1) / 2;
    try {       // (run_pool's own bookkeeping allocates: nothing may leave through the C ABI)
        run_pool(count, threads, [&](int32_t k) {
            try {
                const auto& f = batches[k]->files[(size_t)file_idx[k]];
                std::vector<const char*> ids((size_t)n);
                std::vector<int64_t> lens((size_t)n);
                for (int32_t i = 0; i < n; ++i) { ids[(size_t)i] = f.ids.data() + f.spans[2 * (size_t)i]; lens[(size_t)i] = f.spans[2 * (size_t)i + 1]; }
                const float* p = preds + (size_t)k * P;
                const int64_t need = format_phylip_impl(p, n, ids.data(), lens.data(), nullptr, 0);
                if (need < 0) { status[k] = -EINVAL; return; }
                std::string text((size_t)need, '\0');
                format_phylip_impl(p, n, ids.data(), lens.data(), &text[0], need);
                status[k] = write_file(out_paths[k], text.data(), text.size());
                if (tree_paths && status[k] == 0) {             // <stem>.nj.nwk beside it (infer_alns.py:120-123)
                    nj_newick(p, n, ids.data(), lens.data(), true, text);
                    status[k] = write_file(tree_paths[k], text.data(), text.size());
                }
            } catch (const std::bad_alloc&) { status[k] = -ENOMEM; }
            catch (...) { status[k] = -EIO; }
        });
    } catch (...) { return PF_ENOMEM; }
    return PF_OK;
}

}  // extern "C"

// ---- balanced NNI refinement on the host (pf_bme_nni_host, pf_bme_newick_n; pf_bme_host.h) ------
namespace {

// one source through the serial run of the kernels' bodies (one workgroup of one thread: the results do not depend on
// the geometry); false: an invalid start table
bool bme_one(const float* preds, const int32_t* start, int32_t n, int32_t* slots, double* lengths, int32_t* steps, double* tree_length,
             uint8_t* status) {
    pfbme::Serial run;
    const int epg = (int)pfbme::root_of(n);
    if (!run.setup(preds, start, 1, n, epg)) return false;
    run.run(1, epg, 1, true);
    run.result(0, slots, lengths, steps, tree_length, status);
    return true;
}

// likewise the balanced SPR search
bool spr_one(const float* preds, const int32_t* start, int32_t n, int32_t* slots, double* lengths, int32_t* steps, double* tree_length,
             uint8_t* status) {
    pfbme::SprSerial run;
    if (!run.setup(preds, start, 1, n, (int)pfbme::root_of(n))) return false;
    run.run(1, 1, true);
    run.result(0, slots, lengths, steps, tree_length, status);
    return true;
}

using refine_fn = bool (*)(const float*, const int32_t*, int32_t, int32_t*, double*, int32_t*, double*, uint8_t*);

int refine_host(refine_fn one, const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths,
                int32_t* steps, double* tree_length, uint8_t* status) {
    if (!preds || !start_slots || !slots || !lengths || !steps || !tree_length || !status || B < 1 || N < 3 || N > pfbme::MAX_N)
        return PF_EINVAL;
    const size_t PN = (size_t)N * ((size_t)N - 1) / 2, T = (size_t)pfnj::table_len(N);
    if (PN >= ((size_t)1 << 31)) return PF_EINVAL;
    try {
        std::vector<int32_t> parent((size_t)pfbme::nodes_of(N)), children((size_t)pfbme::nodes_of(N) * 3);
        for (int32_t b = 0; b < B; ++b)                          // refused before any work
            if (!pfbme::tree_of_joins(start_slots + (size_t)b * T, N, parent.data(), children.data())) return PF_EINVAL;
        for (int32_t b = 0; b < B; ++b)
            if (!one(preds + (size_t)b * PN, start_slots + (size_t)b * T, N, slots + (size_t)b * T, lengths + (size_t)b * T, steps + b,
                     tree_length + b, status + b))
                return PF_EINVAL;
        return PF_OK;
    } catch (...) { return PF_ENOMEM; }
}

}  // namespace

extern "C" {

int pf_bme_nni_host(const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths, int32_t* steps,
                    double* tree_length, uint8_t* status) {
    return refine_host(bme_one, preds, start_slots, B, N, slots, lengths, steps, tree_length, status);
}

int pf_bme_spr_host(const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths, int32_t* steps,
                    double* tree_length, uint8_t* status) {
    return refine_host(spr_one, preds, start_slots, B, N, slots, lengths, steps, tree_length, status);
}

}  // extern "C"

namespace {

// the start table of one source; false: a NaN or an infinity in it, and no table
using start_fn = bool (*)(const float*, int32_t, int32_t*, double*);

bool nj_start(const float* preds, int32_t n, int32_t* slots, double* lengths) {
    NjTree t;
    nj_core(preds, n, t);
    table_of_tree(t, slots, lengths);
    return true;
}

bool bionj_start(const float* preds, int32_t n, int32_t* slots, double* lengths) {
    uint8_t bad = 1;
    pfbionj::run_serial(preds, 1, n, slots, lengths, &bad);
    return !bad;
}

// Start, search (`one`, or none: NULL), and the text of the table that comes out, with the number of moves behind it
// (steps_out may be NULL).  The NJ text, after no move, where there is no such table: n < 3, a start that flags its
// source, a search that refuses the start table (a NaN in the distances can leave nj_core with a table that is none) or
// flags its source.
int64_t tree_newick(start_fn start, refine_fn one, const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens,
                    int32_t clamp_negative, char* out, int64_t cap, int32_t* steps_out) {
    if (steps_out) *steps_out = 0;
    if (!preds || (one && n > pfbme::MAX_N)) return PF_EINVAL;          // (the bound is the searches')
    return text_call(n, ids, id_lens, out, cap, [&](std::string& text) {
        const size_t len = n >= 3 ? (size_t)pfnj::table_len(n) : 0;
        std::vector<int32_t> slots(len, 0), found(one ? len : 0);
        std::vector<double> lengths(len, 0.0);
        bool ok = n >= 3 && start(preds, n, slots.data(), lengths.data());
        if (ok && one) {
            int32_t steps = 0;
            double tree_length = 0.0;
            uint8_t status = 0;
            ok = one(preds, slots.data(), n, found.data(), lengths.data(), &steps, &tree_length, &status) && status != pfbme::ST_NONFINITE;
            if (ok && steps_out) *steps_out = steps;
            slots.swap(found);
        }
        if (ok) nj_format(tree_of_table(slots.data(), lengths.data(), n), n, ids, id_lens, clamp_negative != 0, nullptr, text);
        else nj_newick(preds, n, ids, id_lens, clamp_negative != 0, text);
        return PF_OK;
    });
}

}  // namespace

extern "C" {

// pf_bme_newick_n and the number of moves behind the text (bound by phyloformer_amd/hostio.py::bme_newick; not part of
// the public header)
int64_t pf_bme_newick_steps_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                              char* out, int64_t cap, int32_t* steps_out) {
    return tree_newick(nj_start, bme_one, preds, n, ids, id_lens, clamp_negative, out, cap, steps_out);
}

int64_t pf_bme_newick_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                        char* out, int64_t cap) {
    return pf_bme_newick_steps_n(preds, n, ids, id_lens, clamp_negative, out, cap, nullptr);
}

// the same for the balanced SPR search (pf_bme_spr_host); pf_bme_spr_newick_steps_n is bound by hostio.py::spr_newick
int64_t pf_bme_spr_newick_steps_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                                  char* out, int64_t cap, int32_t* steps_out) {
    return tree_newick(nj_start, spr_one, preds, n, ids, id_lens, clamp_negative, out, cap, steps_out);
}

int64_t pf_bme_spr_newick_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                            char* out, int64_t cap) {
    return pf_bme_spr_newick_steps_n(preds, n, ids, id_lens, clamp_negative, out, cap, nullptr);
}

}  // extern "C"

extern "C" {

// Bootstrap supports (bound by phyloformer_amd/hostio.py::nj_support; not part of the public header): the pf_nj_newick_n
// text of preds [n(n-1)/2] with, after the ')' of every internal node, the integer percent (200 c + R) / (2 R) of the
// R replicate trees of reps [R][n(n-1)/2] that contain the node's split.  The replicates are joined on up to `threads`
// threads.  Twin of phyloformer_amd/bootstrap.py::support_newick_py, byte for byte.  Sizing protocol as
// pf_format_phylip; every call joins all R replicates, so size with pf_nj_newick_n (the labels add at most 3 bytes
// per internal node).
int64_t pf_nj_support_n(const float* preds, const float* reps, int32_t R, int32_t n, const char* const* ids,
                        const int64_t* id_lens, int32_t clamp_negative, int32_t threads, char* out, int64_t cap) {
    if (!preds || !reps || R < 1) return PF_EINVAL;
    return text_call(n, ids, id_lens, out, cap, [&](std::string& text) {
        if (n <= 3) {                               // no internal split
            nj_newick(preds, n, ids, id_lens, clamp_negative != 0, text);
        } else {
            const size_t P = (size_t)n * (size_t)(n - 1) / 2, W = ((size_t)n + 63) / 64;
            NjTree tree;
            nj_core(preds, n, tree);
            std::vector<uint64_t> splits;
            nj_splits(tree, n, splits);
            const size_t S = tree.joins.size();
            std::vector<uint8_t> hit((size_t)R * S, 0);
            std::atomic<bool> failed{false};
            run_pool(R, threads, [&](int32_t r) {
                try {
                    NjTree rt;
                    nj_core(reps + (size_t)r * P, n, rt);
                    std::vector<uint64_t> rs;
                    nj_splits(rt, n, rs);
                    // sorted replicate splits, then one binary search per split of the tree
                    std::vector<size_t> order(rt.joins.size());
                    for (size_t s = 0; s < order.size(); ++s) order[s] = s;
                    auto less = [&](const uint64_t* x, const uint64_t* y) {
                        return std::lexicographical_compare(x, x + W, y, y + W);
                    };
                    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return less(&rs[x * W], &rs[y * W]); });
                    for (size_t s = 0; s < S; ++s) {
                        const uint64_t* key = &splits[s * W];
                        auto it = std::lower_bound(order.begin(), order.end(), key,
                                                   [&](size_t x, const uint64_t* k) { return less(&rs[x * W], k); });
                        hit[(size_t)r * S + s] = it != order.end() && std::equal(key, key + W, &rs[*it * W]);
                    }
                } catch (...) { failed = true; }
            });
            if (failed) return PF_ENOMEM;
            std::vector<int32_t> support(S);
            for (size_t s = 0; s < S; ++s) {
                int64_t c = 0;
                for (int32_t r = 0; r < R; ++r) c += hit[(size_t)r * S + s];
                support[s] = (int32_t)((200 * c + R) / (2 * (int64_t)R));
            }
            nj_format(tree, n, ids, id_lens, clamp_negative != 0, support.data(), text);
        }
        return PF_OK;
    });
}

}  // extern "C"

extern "C" {

// The join tables of pf_nj_joins without a device (bound by phyloformer_amd/hostio.py::nj_joins_host; not part of the
// public header): nj_core's joins of preds [B][P_N] as slots / lengths [B][2 (N - 3) + 3], on up to `threads` threads.  A
// source with a NaN or an infinity is flagged and its table zeros.
int pf_nj_joins_host_n(const float* preds, int32_t B, int32_t N, int32_t threads, int32_t* slots, double* lengths, uint8_t* nonfinite) {
    if (!preds || !slots || !lengths || !nonfinite || B < 1 || N < 3) return PF_EINVAL;
    const size_t P = (size_t)N * ((size_t)N - 1) / 2, T = (size_t)pfnj::table_len(N);
    std::atomic<bool> failed{false};
    try {
        run_pool(B, threads, [&](int32_t b) {
            try {
                const float* p = preds + (size_t)b * P;
                int32_t* s = slots + (size_t)b * T;
                double* l = lengths + (size_t)b * T;
                bool bad = false;
                for (size_t e = 0; e < P; ++e) bad |= !(p[e] - p[e] == 0.0f);
                nonfinite[b] = bad;
                if (bad) { std::fill(s, s + T, 0); std::fill(l, l + T, 0.0); return; }
                NjTree t;
                nj_core(p, N, t);
                table_of_tree(t, s, l);
            } catch (...) { failed = true; }
        });
    } catch (...) { return PF_ENOMEM; }
    return failed ? PF_ENOMEM : PF_OK;
}

// BIONJ without a device: the bodies of pf_bionj.hip.h's kernels run serially, one source at a
// time - the same tables as pf_bionj_joins, bit for bit.  Twin of phyloformer_amd/bionj.py::bionj_joins.  A source with
// a NaN or an infinity is flagged and its table zeros.
int pf_bionj_joins_host(const float* preds, int32_t B, int32_t N, int32_t* slots, double* lengths, uint8_t* nonfinite) {
    if (!preds || !slots || !lengths || !nonfinite || B < 1 || N < 3) return PF_EINVAL;
    const size_t P = (size_t)N * ((size_t)N - 1) / 2, T = (size_t)pfnj::table_len(N);
    if (P >= ((size_t)1 << 31)) return PF_EINVAL;
    try {
        for (int32_t b = 0; b < B; ++b) {
            int32_t* s = slots + (size_t)b * T;
            double* l = lengths + (size_t)b * T;
            std::fill(s, s + T, 0);
            std::fill(l, l + T, 0.0);
            pfbionj::run_serial(preds + (size_t)b * P, 1, N, s, l, nonfinite + b);
        }
        return PF_OK;
    } catch (...) { return PF_ENOMEM; }
}

// Delta scores without a device: every quartet of every source once, serially - the same arrays
// as pf_delta, bit for bit.  Twin of phyloformer_amd/delta.py::delta_py.  A source with a NaN or an infinity is flagged
// and its arrays zeros.
int pf_delta_host(const float* preds, int32_t B, int32_t N, int32_t K, int64_t* pair_sum, int64_t* hist, uint8_t* nonfinite) {
    if (!preds || !pair_sum || !hist || !nonfinite || pfdelta::refused(B, N, K)) return PF_EINVAL;
    const size_t P = (size_t)N * ((size_t)N - 1) / 2;
    for (int32_t b = 0; b < B; ++b)
        pfdelta::run_serial(preds + (size_t)b * P, N, K, pair_sum + (size_t)b * P, hist + (size_t)b * (size_t)K, nonfinite + b);
    return PF_OK;
}

// Least-squares branch lengths without a device: every tree of every source serially - the same
// arrays as pf_tree_ols, bit for bit.  Twin of phyloformer_amd/ols.py::tree_ols_py.  A tree with a status has zeros.
int pf_tree_ols_host(const float* preds, const int32_t* slots, int32_t B, int32_t M, int32_t N, double* ols, uint8_t* status) {
    if (!preds || !slots || !ols || !status || pfols::refused(B, M, N)) return PF_EINVAL;
    try {
        const size_t n = (size_t)N, P = n * (n - 1) / 2, T = (size_t)pfols::table_len(N);
        for (size_t b = 0; b < (size_t)B; ++b)
            for (size_t m = 0; m < (size_t)M; ++m) {
                const size_t item = b * (size_t)M + m;
                pfols::run_serial(preds + b * P, slots + item * T, N, ols + item * T, status + item);
            }
        return PF_OK;
    } catch (...) { return PF_ENOMEM; }
}

// Tree rooting without a device: every tree serially - the same arrays as pf_tree_root, bit for bit.
// Twin of phyloformer_amd/root.py::tree_root_py.  A tree with a status has zeros.
int pf_tree_root_host(const int32_t* slots, const double* lengths, int32_t B, int32_t M, int32_t N, double* ssq, double* pos, double* mid,
                      uint8_t* status) {
    if (!slots || !lengths || !ssq || !pos || !mid || !status || pfroot::refused(B, M, N)) return PF_EINVAL;
    try {
        const size_t T = (size_t)pfroot::table_len(N), items = (size_t)B * (size_t)M;
        for (size_t item = 0; item < items; ++item)
            pfroot::run_serial(slots + item * T, lengths + item * T, N, ssq + item * T, pos + item * T, mid + item * pfroot::MID, status + item);
        return PF_OK;
    } catch (...) { return PF_ENOMEM; }
}

// Tree fit without a device: every tree of every source serially - the same arrays as pf_tree_fit,
// bit for bit.  Twin of phyloformer_amd/fit.py::tree_fit_py.  A tree with a status has zeros everywhere.
int pf_tree_fit_host(const float* preds, const int32_t* slots, const double* lengths, int32_t B, int32_t M, int32_t N, double* patristic,
                     double* rows, int32_t* worst_j, uint8_t* status) {
    if (!preds || !slots || !lengths || !rows || !worst_j || !status || pffit::refused(B, M, N)) return PF_EINVAL;
    try {
        const size_t n = (size_t)N, P = n * (n - 1) / 2, T = (size_t)pffit::table_len(N);
        for (size_t b = 0; b < (size_t)B; ++b)
            for (size_t m = 0; m < (size_t)M; ++m) {
                const size_t item = b * (size_t)M + m;
                pffit::run_serial(preds + b * P, slots + item * T, lengths + item * T, N, patristic ? patristic + item * P : nullptr,
                                  rows + item * n * pffit::COLS, worst_j + item * n, status + item);
            }
        return PF_OK;
    } catch (...) { return PF_ENOMEM; }
}

// preds [n(n-1)/2] -> Newick text of the BIONJ tree, as bionj.py::bionj_newick_py writes it: pf_bionj_joins_host's table
// through pf_nj_format_joins_n's writer.  n < 3 or a NaN / infinity in preds: pf_nj_newick_n's text.
int64_t pf_bionj_newick_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                          char* out, int64_t cap) {
    return tree_newick(bionj_start, nullptr, preds, n, ids, id_lens, clamp_negative, out, cap, nullptr);
}

// pf_join_supports_host, and with `x` (its arg is set here) pf_join_transfers_host: the bodies of pf_support.hip.h's
// kernels run serially, one source at a time.  What only the transfers refuse stands at their call.
static int join_supports_host(const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R, int32_t N,
                              int32_t* count, int64_t* transfer, int32_t* depth, uint8_t* status, pfsup::Transfers* x) {
    if (!ref_slots || !rep_slots || !count || !transfer || !depth || !status || B < 1 || R < 1 || N < 4 || N > pfbme::MAX_N)
        return PF_EINVAL;
    const size_t T = (size_t)pfnj::table_len(N), S = (size_t)N - 3, W = (size_t)pfsup::words_of(N), b = (size_t)B, r = (size_t)R;
    size_t total = 0;
    if (__builtin_mul_overflow(b * r, T * sizeof(int32_t), &total)) return PF_EINVAL;
    try {
        std::vector<int32_t> parent((size_t)pfbme::nodes_of(N)), children((size_t)pfbme::nodes_of(N) * 3);
        for (size_t i = 0; i < b; ++i)                            // refused before any work
            if (!pfbme::tree_of_joins(ref_slots + i * T, N, parent.data(), children.data())) return PF_EINVAL;
        for (size_t i = 0; i < b * r; ++i)
            if (!(rep_flag && rep_flag[i]) && !pfbme::tree_of_joins(rep_slots + i * T, N, parent.data(), children.data())) return PF_EINVAL;
        // the state of one source with all its replicates, reused from source to source
        std::vector<uint64_t> bits((r + 1) * S * W), tile((size_t)pfsup::TILE * W);
        std::vector<int32_t> row((r + 1) * (size_t)N), sizes(S), delta(r * S), arg(x ? r * S : 0);
        std::vector<uint8_t> bad(b * (r + 1), 0);
        pfsup::Args a{};
        a.ref_slots = ref_slots; a.rep_slots = rep_slots; a.rep_flag = rep_flag;
        a.bits = bits.data(); a.row = row.data(); a.sizes = sizes.data(); a.delta = delta.data(); a.bad = bad.data();
        a.count = count; a.transfer = transfer; a.depth = depth; a.status = status;
        a.N = N; a.R = R; a.nb = 1; a.r0 = 0; a.rc = R;
        if (x) x->arg = arg.data();
        for (int32_t src = 0; src < B; ++src) {
            a.b0 = src;
            if (x) pfsup::serial_chunk<true>(a, tile.data(), true, x);
            else pfsup::serial_chunk(a, tile.data(), true);
        }
        return PF_OK;
    } catch (...) { return PF_ENOMEM; }
}

// Split supports without a device: the same integers as pf_join_supports.  Twin of
// phyloformer_amd/supports.py::split_supports.
int pf_join_supports_host(const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R, int32_t N,
                          int32_t* count, int64_t* transfer, int32_t* depth, uint8_t* status) {
    return join_supports_host(ref_slots, rep_slots, rep_flag, B, R, N, count, transfer, depth, status, nullptr);
}

// Per-taxon transfer counts without a device: pf_join_supports_host's run with the matching that
// keeps its keys, and k_sup_moves' body after it.  Twin of phyloformer_amd/supports.py::transfer_taxa.
int pf_join_transfers_host(const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R, int32_t N,
                           int32_t cutoff_percent, int32_t* count, int64_t* transfer, int32_t* depth, int64_t* moves, int32_t* used,
                           int32_t* capped, int32_t* branch_moves, uint8_t* status) {
    if (!moves || !used || !capped || cutoff_percent < 0 || cutoff_percent > 100) return PF_EINVAL;
    size_t total = 0;       // (B < 1 or N < 4 wrap the product and are refused whatever it gives)
    if (branch_moves && __builtin_mul_overflow((size_t)B * ((size_t)N - 3), (size_t)N * sizeof(int32_t), &total)) return PF_EINVAL;
    pfsup::Transfers x{nullptr, moves, used, capped, branch_moves, cutoff_percent};
    return join_supports_host(ref_slots, rep_slots, rep_flag, B, R, N, count, transfer, depth, status, &x);
}

// Majority-rule consensus without a device: the bodies of pf_consensus.hip.h's kernels run
// serially, one source at a time - the same integers and the same doubles as pf_join_consensus.  Tables are checked by
// the bodies themselves, as pf_join_consensus_device's are: a source with a table that is no join table gets status 1
// and zeros.  Twin of phyloformer_amd/consensus.py::join_consensus.
int pf_join_consensus_host(const int32_t* rep_slots, const double* rep_lengths, const uint8_t* rep_flag, int32_t B, int32_t R, int32_t N,
                           int32_t percent, int32_t* n_splits, int32_t* count, int32_t* size, int32_t* parent, double* split_length,
                           int32_t* leaf_parent, double* leaf_length, uint8_t* status) {
    if (!rep_slots || !n_splits || !count || !size || !parent || !leaf_parent || !status || (rep_lengths && (!split_length || !leaf_length)) ||
        B < 1 || R < 1 || N < 4 || N > pfbme::MAX_N || percent < 50 || percent > 99 || (int64_t)R * ((int64_t)N - 3) > pfcon::MAX_ENTRIES)
        return PF_EINVAL;
    const size_t T = (size_t)pfnj::table_len(N), S = (size_t)N - 3, W = (size_t)pfsup::words_of(N), b = (size_t)B, r = (size_t)R;
    size_t total = 0;
    if (__builtin_mul_overflow(b * r, T * sizeof(double), &total)) return PF_EINVAL;
    try {
        pfcon::Args a{};
        a.rep_slots = rep_slots; a.rep_lengths = rep_lengths; a.rep_flag = rep_flag;
        a.n_splits = n_splits; a.count = count; a.size = size; a.parent = parent; a.leaf_parent = leaf_parent;
        a.split_length = split_length; a.leaf_length = leaf_length; a.status = status;
        a.N = N; a.R = R; a.percent = percent; a.nb = 1;
        a.cap = pfcon::capacity_of((int64_t)(r * S));
        std::fill(n_splits, n_splits + b, 0);
        std::fill(count, count + b * S, 0);
        std::fill(size, size + b * S, 0);
        std::fill(parent, parent + b * S, 0);
        std::fill(leaf_parent, leaf_parent + b * (size_t)N, 0);
        if (rep_lengths) { std::fill(split_length, split_length + b * S, 0.0); std::fill(leaf_length, leaf_length + b * (size_t)N, 0.0); }
        // the state of one source, reused from source to source
        std::vector<unsigned char> state(pfcon::state_bytes(N, R, rep_lengths != nullptr));
        std::vector<uint64_t> tile((size_t)pfcon::TILE * W);
        pfspan::Carve c{reinterpret_cast<char*>(state.data())};
        pfcon::state_arrays(c, a, 1, r, N, (size_t)a.cap, rep_lengths != nullptr);
        char *ones = reinterpret_cast<char*>(a.slot_of), *zeros = reinterpret_cast<char*>(a.tally);
        for (int32_t src = 0; src < B; ++src) {
            a.b0 = src;
            std::fill(ones, zeros, (char)0xff);
            std::fill(zeros, c.at, (char)0);
            pfcon::serial_source(a, 0, tile.data());
        }
        return PF_OK;
    } catch (...) { return PF_ENOMEM; }
}

// Tree distances without a device: the bodies of pf_treedist.hip.h's kernels run serially, one
// source at a time - the same integers and the same doubles as pf_join_distances.  Tables are checked by the bodies
// themselves, as pf_join_distances_device's are: a source with a table that is no join table gets status 1 and zeros.
// Twin of phyloformer_amd/treedist.py::join_distances_py.
int pf_join_distances_host(const int32_t* slots, const double* lengths, const uint8_t* flag, int32_t B, int32_t K, int32_t N,
                           int32_t* shared, double* kf, double* wrf, uint8_t* status) {
    if (!slots || !shared || !status || (lengths && (!kf || !wrf)) || B < 1 || K < 1 || K > pftd::MAX_K || N < pftd::MIN_N ||
        N > pftd::MAX_N)
        return PF_EINVAL;
    const size_t T = (size_t)pfnj::table_len(N), b = (size_t)B, k = (size_t)K;
    size_t total = 0;
    if (__builtin_mul_overflow(b * k, T * sizeof(double), &total) || __builtin_mul_overflow(b * k, k * sizeof(double), &total)) return PF_EINVAL;
    try {
        pftd::Args a{};
        a.c.rep_slots = slots; a.c.rep_lengths = lengths; a.c.rep_flag = flag; a.c.status = status;
        a.c.N = N; a.c.R = K; a.c.nb = 1;
        a.c.cap = pfcon::capacity_of((int64_t)K * ((int64_t)N - 3));
        a.shared = shared; a.kf = kf; a.wrf = wrf;
        std::fill(shared, shared + b * k * k, 0);
        if (lengths) { std::fill(kf, kf + b * k * k, 0.0); std::fill(wrf, wrf + b * k * k, 0.0); }
        // the state of one source, reused from source to source
        std::vector<unsigned char> state(pftd::state_bytes(N, K));
        pfspan::Carve c{reinterpret_cast<char*>(state.data())};
        pftd::state_arrays(c, a, 1, k, N, (size_t)a.c.cap);
        char *ones = reinterpret_cast<char*>(a.c.slot_of), *zeros = reinterpret_cast<char*>(a.c.tally);
        for (int32_t src = 0; src < B; ++src) {
            a.c.b0 = src;
            std::fill(ones, zeros, (char)0xff);
            std::fill(zeros, c.at, (char)0);
            pftd::serial_source(a, 0);
        }
        return PF_OK;
    } catch (...) { return PF_ENOMEM; }
}

}  // extern "C"
