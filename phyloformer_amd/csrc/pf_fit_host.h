// Tree fit (pf_tree_fit, pf_tree_fit_device, pf_tree_fit_host): the path-length (patristic) distances of
// a join table and the sums of their residuals against the distances the tree was built from.  Plain C++, no HIP:
// tests/native/pf_fit_main.cpp runs the serial twin under AddressSanitizer / UBSan, pf_fit.hip.h compiles the bodies for the
// device too (PF_TAXA_HD).  phyloformer_amd/fit.py is the statement: every float64 operation here happens with the same
// operands and in the same order as there, nothing contracts (the bodies switch contraction off; a g++ build passes
// -ffp-contract=off), so the arrays are bit-identical.
//
// Nodes: leaves 0 .. N-1; join t makes node N + t over the nodes then in slots a and b (branches lengths[2t], lengths[2t+1]),
// slot a standing for it afterwards; node 2N - 3 is the parent of the last three.  A parent's number is above its children's,
// so the walk from two leaves that always advances the lower-numbered node meets at the lowest common node.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pf_spans.h"
#include "pf_taxa_host.h"

namespace pffit {

constexpr int MIN_N = 3, MAX_N = 8192;     // the setup kernel keeps the table and one int32 per slot in LDS: 98,292 bytes at the cap
constexpr int LANES = 64, COLS = 6;        // rows: ss, fm, st, stt, sdt, worst
constexpr uint8_t OK = 0, NONFINITE = 1, NO_TABLE = 2;

PF_TAXA_HD constexpr int table_len(int N) { return 2 * (N - 3) + 3; }
PF_TAXA_HD constexpr int nodes_of(int N) { return 2 * N - 2; }
PF_TAXA_HD inline bool nonfinite(double x) { return !(x - x == 0.0); }
PF_TAXA_HD inline int64_t row_start(int64_t i, int64_t n) { return i * (2 * n - i - 1) / 2; }
// index of the pair of i != j among n sequences
PF_TAXA_HD inline int64_t pair_at(int i, int j, int n) {
    return i < j ? row_start(i, n) + (j - i - 1) : row_start(j, n) + (i - j - 1);
}

// what the three entry points refuse about (B, M, N): 0, or which (1: N below, 2: N above, 3: B, 4: M, 5: the pairs)
inline int refused(int B, int M, int N) {
    if (N < MIN_N) return 1;
    if (N > MAX_N) return 2;
    if (B < 1) return 3;
    if (M < 1) return 4;
    if ((int64_t)N * (N - 1) / 2 >= ((int64_t)1 << 31)) return 5;
    return 0;
}

// The table replayed by ONE thread: parent / len [2N - 2] of its nodes; `node` [N] is scratch (the node in every slot,
// -1 once the slot has left).  NO_TABLE for a slot outside [0, N), a slot joined after it left, a == b - nothing is read or
// written out of bounds for any table -, else OK.  The last node is its own parent, length 0.
PF_TAXA_HD inline uint8_t replay(const int32_t* slots, const double* lengths, int N, int32_t* node, int32_t* parent, double* len) {
    for (int s = 0; s < N; ++s) node[s] = s;
    const int J = N - 3, root = 2 * N - 3;
    for (int t = 0; t < J; ++t) {
        const int32_t a = slots[2 * t], b = slots[2 * t + 1];
        if (a < 0 || a >= N || b < 0 || b >= N || a == b || node[a] < 0 || node[b] < 0) return NO_TABLE;
        parent[node[a]] = N + t; len[node[a]] = lengths[2 * t];
        parent[node[b]] = N + t; len[node[b]] = lengths[2 * t + 1];
        node[a] = N + t; node[b] = -1;
    }
    for (int k = 0; k < 3; ++k) {
        const int32_t s = slots[2 * J + k];
        if (s < 0 || s >= N || node[s] < 0) return NO_TABLE;      // (a repeated slot has left by its second use)
        parent[node[s]] = root; len[node[s]] = lengths[2 * J + k];
        node[s] = -1;
    }
    parent[root] = root; len[root] = 0.0;
    return OK;
}

// T[x, y] of leaves x != y of a replayed table: two sums from +0.0, each in walking order, then their sum
PF_TAXA_HD inline double walk(const int32_t* parent, const double* len, int x, int y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int u = x, v = y;
    double su = 0.0, sv = 0.0;
    while (u != v) {
        if (u < v) { su = su + len[u]; u = parent[u]; }
        else { sv = sv + len[v]; v = parent[v]; }
    }
    return su + sv;
}

// One of the 64 strided accumulators of a row.
struct Acc {
    double ss, fm, st, stt, sdt, worst;
    int32_t wj;
};
PF_TAXA_HD inline Acc acc_none(int N) { return Acc{0.0, 0.0, 0.0, 0.0, 0.0, -1.0, N}; }

// partner j of the row: the distance d = pred (float32) and the tree's t
PF_TAXA_HD inline void acc_take(Acc& a, float pred, double t, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = (double)pred;
    const double e = d - t;
    const double e2 = e * e;
    double q = 0.0;
    if (d > 0.0) { const double d2 = d * d; q = e2 / d2; }
    const double tt = t * t, dt = d * t;
    a.ss = a.ss + e2;
    a.fm = a.fm + q;
    a.st = a.st + t;
    a.stt = a.stt + tt;
    a.sdt = a.sdt + dt;
    const double m = fabs(e);
    if (m > a.worst) { a.worst = m; a.wj = j; }
}

// lane l takes lane l + s
PF_TAXA_HD inline void acc_merge(Acc& a, const Acc& o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    a.ss = a.ss + o.ss;
    a.fm = a.fm + o.fm;
    a.st = a.st + o.st;
    a.stt = a.stt + o.stt;
    a.sdt = a.sdt + o.sdt;
    if (o.worst > a.worst || (o.worst == a.worst && o.wj < a.wj)) { a.worst = o.worst; a.wj = o.wj; }
}

// lane `lane` of row i: partners j = lane, lane + 64, ... but i, ascending; tree [P_N] in pair order
PF_TAXA_HD inline Acc row_lane(const float* pred, const double* tree, int N, int i, int lane) {
    Acc a = acc_none(N);
    for (int j = lane; j < N; j += LANES) {
        if (j == i) continue;
        const int64_t p = pair_at(i, j, N);
        acc_take(a, pred[p], tree[p], j);
    }
    return a;
}

PF_TAXA_HD inline void row_store(const Acc& a, double* row, int32_t* wj) {
    row[0] = a.ss; row[1] = a.fm; row[2] = a.st; row[3] = a.stt; row[4] = a.sdt; row[5] = a.worst;
    *wj = a.wj;
}

// One tree of one source, serially: patristic [P_N] or null, rows [N][6], worst_j [N] (all zeroed here), the status.
inline void run_serial(const float* pred, const int32_t* slots, const double* lengths, int N, double* patristic, double* rows,
                       int32_t* worst_j, uint8_t* status) {
    const int64_t n = N, P = n * (n - 1) / 2;
    const int T = table_len(N);
    if (patristic) for (int64_t e = 0; e < P; ++e) patristic[e] = 0.0;
    for (int64_t e = 0; e < n * COLS; ++e) rows[e] = 0.0;
    for (int i = 0; i < N; ++i) worst_j[i] = 0;
    std::vector<int32_t> node((size_t)N), parent((size_t)nodes_of(N));
    std::vector<double> len((size_t)nodes_of(N));
    *status = replay(slots, lengths, N, node.data(), parent.data(), len.data());
    if (*status != OK) return;
    bool bad = false;
    for (int64_t e = 0; e < P; ++e) bad |= nonfinite((double)pred[e]);
    for (int k = 0; k < T; ++k) bad |= nonfinite(lengths[k]);
    if (bad) { *status = NONFINITE; return; }
    std::vector<double> own;
    if (!patristic) { own.resize((size_t)P); patristic = own.data(); }
    int64_t p = 0;
    for (int x = 0; x < N; ++x)
        for (int y = x + 1; y < N; ++y, ++p) patristic[p] = walk(parent.data(), len.data(), x, y);
    Acc lanes[LANES];
    for (int i = 0; i < N; ++i) {
        for (int l = 0; l < LANES; ++l) lanes[l] = row_lane(pred, patristic, N, i, l);
        for (int s = LANES / 2; s > 0; s >>= 1)
            for (int l = 0; l < s; ++l) acc_merge(lanes[l], lanes[l + s]);
        row_store(lanes[0], rows + (size_t)i * COLS, worst_j + i);
    }
}

// The arrays of a call as the caller or the staging of a host call holds them: B sources of M trees each.
struct Tables {
    const float* preds; const int32_t* slots; const double* lengths;
    double* patristic; double* rows; int32_t* worst_j; uint8_t* status;
};
template <class V>
inline void staging_arrays(V& v, Tables& s, const Tables& u, size_t B, size_t M, int N) {
    const size_t n = (size_t)(N > 0 ? N : 0), P = n * (n > 0 ? n - 1 : 0) / 2, T = (size_t)(N >= 3 ? table_len(N) : 0);
    v.in(s.lengths, u.lengths, B * M * T);
    v.out(s.patristic, u.patristic, B * M * P, u.patristic ? pfspan::REQUIRED : pfspan::ABSENT);
    v.out(s.rows, u.rows, B * M * n * COLS);
    v.in(s.preds, u.preds, B * P);
    v.in(s.slots, u.slots, B * M * T);
    v.out(s.worst_j, u.worst_j, B * M * n);
    v.out(s.status, u.status, B * M);
}

}  // namespace pffit
