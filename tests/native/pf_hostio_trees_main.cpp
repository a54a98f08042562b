// Stand-alone driver of the tree half of csrc/pf_hostio.cpp for AddressSanitizer / UBSan builds
// (tests/test_hostio_trees_native.py), compiled together with it; every buffer is an exactly sized heap array.
//
//     pf_hostio_trees_main text N clamp preds.bin
//         preds.bin: float [P_N].  The frame of every text entry point - capacities 0, need - 1 and need, and every
//         refusal - is checked here (exit code 1 and a line on stderr for a miss).  The table round trip
//         pf_nj_joins_host_n -> pf_nj_format_joins_n is compared with pf_nj_newick_n.  Printed: "== name steps bytes\n"
//         and the text, for nj, joins, bionj, bme and spr; ids() below gives the ids.
//     pf_hostio_trees_main supports B R N cutoff tables.bin
//         tables.bin: ref int32 [B][T], rep int32 [B][R][T], flag uint8 [B][R].  Printed: "name flags branch_moves:" and
//         the integers of every result of pf_join_supports_host and pf_join_transfers_host, with and without the flags
//         and branch_moves.
//
// Exit code 0 = done, 1 = a check missed, 2 = usage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/phyloformer_amd.h"

extern "C" {
int64_t pf_nj_support_n(const float*, const float*, int32_t, int32_t, const char* const*, const int64_t*, int32_t, int32_t, char*, int64_t);
int64_t pf_bme_newick_steps_n(const float*, int32_t, const char* const*, const int64_t*, int32_t, char*, int64_t, int32_t*);
int64_t pf_bme_spr_newick_steps_n(const float*, int32_t, const char* const*, const int64_t*, int32_t, char*, int64_t, int32_t*);
int pf_nj_joins_host_n(const float*, int32_t, int32_t, int32_t, int32_t*, double*, uint8_t*);
}

namespace {

int misses = 0;
void expect(bool ok, const char* what, const char* who) {
    if (!ok) { fprintf(stderr, "MISS %s: %s\n", who, what); ++misses; }
}

template <class T>
bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(v.data(), sizeof(T), v.size(), f) == v.size() && fgetc(f) == EOF;
    fclose(f);
    return ok;
}

// an empty id, a NUL byte, multi-byte UTF-8, then plain ones
std::vector<std::string> ids(int n) {
    std::vector<std::string> out;
    for (int i = 0; i < n; ++i) {
        if (i == 0) out.push_back("");
        else if (i == 1) out.push_back(std::string("a\0b", 3));
        else if (i == 2) out.push_back("\xc3\xa9\xe6\x97\xa5");
        else out.push_back("t" + std::to_string(i));
    }
    return out;
}

// A text call with everything but (out, cap) bound: the three capacities of the sizing protocol on exactly sized
// buffers.  Returns the text ("" after a miss).
template <class Call>
std::string sized(const char* who, Call&& call) {
    const int64_t need = call(nullptr, 0);
    expect(need > 0, "the query returns the size", who);
    if (need <= 0) return "";
    std::unique_ptr<char[]> small(new char[(size_t)need - 1]);
    memset(small.get(), 0x7f, (size_t)need - 1);
    expect(call(small.get(), need - 1) == need, "need - 1 bytes: the size again", who);
    bool untouched = true;
    for (int64_t i = 0; i < need - 1; ++i) untouched = untouched && small[(size_t)i] == 0x7f;
    expect(untouched, "need - 1 bytes: nothing written", who);
    std::unique_ptr<char[]> exact(new char[(size_t)need]);
    expect(call(exact.get(), need) == need, "need bytes: the size", who);
    expect(call(nullptr, need) == PF_EINVAL, "no buffer and a capacity: refused", who);
    return std::string(exact.get(), (size_t)need);
}

void print_text(const char* name, int steps, const std::string& text) {
    printf("== %s %d %zu\n", name, steps, text.size());
    fwrite(text.data(), 1, text.size(), stdout);
}

int text_mode(int n, int clamp, const char* path) {
    const size_t P = (size_t)n * (size_t)(n - 1) / 2, T = 2 * ((size_t)n - 3) + 3;
    std::vector<float> preds(P);
    if (!read_all(path, preds)) return 2;
    const std::vector<std::string> names = ids(n);
    std::vector<const char*> id(names.size());
    std::vector<int64_t> len(names.size()), neg;
    for (size_t i = 0; i < names.size(); ++i) { id[i] = names[i].data(); len[i] = (int64_t)names[i].size(); }
    neg = len;
    neg[(size_t)n / 2] = -1;
    const float* p = preds.data();
    const char* const* I = id.data();
    const int64_t* L = len.data();
    char byte = 0;
    const int32_t big = 16384 + 1;                     // pfbme::MAX_N + 1: refused before anything is read

    // the distance calls that share one shape of arguments
    using plain_fn = int64_t (*)(const float*, int32_t, const char* const*, const int64_t*, int32_t, char*, int64_t);
    const struct { const char* name; plain_fn fn; bool bounded; } plain[] = {
        {"nj", pf_nj_newick_n, false}, {"bionj", pf_bionj_newick_n, false}, {"bme", pf_bme_newick_n, true}, {"spr", pf_bme_spr_newick_n, true}};
    std::string texts[4];
    for (int k = 0; k < 4; ++k) {
        const plain_fn fn = plain[k].fn;
        const char* who = plain[k].name;
        texts[k] = sized(who, [&](char* out, int64_t cap) { return fn(p, n, I, L, clamp, out, cap); });
        expect(fn(nullptr, n, I, L, clamp, &byte, 1) == PF_EINVAL, "null preds", who);
        expect(fn(p, n, nullptr, L, clamp, &byte, 1) == PF_EINVAL, "null ids", who);
        expect(fn(p, n, I, nullptr, clamp, &byte, 1) == PF_EINVAL, "null id_lens", who);
        expect(fn(p, n, I, neg.data(), clamp, &byte, 1) == PF_EINVAL, "a negative id length", who);
        expect(fn(p, 0, I, L, clamp, &byte, 1) == PF_EINVAL, "n = 0", who);
        if (plain[k].bounded) expect(fn(p, big, I, L, clamp, &byte, 1) == PF_EINVAL, "n above MAX_N", who);
    }
    // the two with the number of moves: the same text, steps set on every path
    using steps_fn = int64_t (*)(const float*, int32_t, const char* const*, const int64_t*, int32_t, char*, int64_t, int32_t*);
    const steps_fn with_steps[] = {pf_bme_newick_steps_n, pf_bme_spr_newick_steps_n};
    int32_t steps[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        const char* who = k ? "spr steps" : "bme steps";
        int32_t s = -7;
        std::string text(texts[2 + k].size(), '\0');                 // (the capacities are checked above: one run here)
        expect(with_steps[k](p, n, I, L, clamp, &text[0], (int64_t)text.size(), &s) == (int64_t)text.size() && text == texts[2 + k],
               "the text of the call without steps", who);
        expect(s >= 0 && (n > 3 || s == 0), "steps >= 0, and 0 where nothing can move", who);
        steps[k] = s;
        s = -7;
        expect(with_steps[k](p, n, I, L, clamp, nullptr, 1, &s) == PF_EINVAL && s == 0, "no buffer and a capacity leaves steps = 0", who);
        s = -7;
        expect(with_steps[k](p, n, I, neg.data(), clamp, &byte, 1, &s) == PF_EINVAL && s == 0, "a refusal leaves steps = 0", who);
        s = -7;
        expect(with_steps[k](p, big, I, L, clamp, &byte, 1, &s) == PF_EINVAL && s == 0, "n above MAX_N leaves steps = 0", who);
    }

    // table round trip: nj_core -> table_of_tree -> tree_of_table -> the text of pf_nj_newick_n
    std::vector<int32_t> slots(T), bad;
    std::vector<double> lengths(T);
    uint8_t flag = 9;
    expect(pf_nj_joins_host_n(p, 1, n, 1, slots.data(), lengths.data(), &flag) == PF_OK && flag == 0, "pf_nj_joins_host_n", "joins");
    const std::string joined = sized("joins", [&](char* out, int64_t cap) {
        return pf_nj_format_joins_n(slots.data(), lengths.data(), n, I, L, clamp, out, cap); });
    expect(joined == texts[0], "the table's text is pf_nj_newick_n's", "joins");
    expect(pf_nj_format_joins_n(nullptr, lengths.data(), n, I, L, clamp, &byte, 1) == PF_EINVAL, "null slots", "joins");
    expect(pf_nj_format_joins_n(slots.data(), nullptr, n, I, L, clamp, &byte, 1) == PF_EINVAL, "null lengths", "joins");
    expect(pf_nj_format_joins_n(slots.data(), lengths.data(), n, nullptr, L, clamp, &byte, 1) == PF_EINVAL, "null ids", "joins");
    expect(pf_nj_format_joins_n(slots.data(), lengths.data(), n, I, nullptr, clamp, &byte, 1) == PF_EINVAL, "null id_lens", "joins");
    expect(pf_nj_format_joins_n(slots.data(), lengths.data(), n, I, neg.data(), clamp, &byte, 1) == PF_EINVAL, "a negative id length", "joins");
    expect(pf_nj_format_joins_n(slots.data(), lengths.data(), 2, I, L, clamp, &byte, 1) == PF_EINVAL, "n = 2", "joins");
    for (const int32_t v : {-1, n}) {
        bad = slots;
        bad[T - 1] = v;
        expect(pf_nj_format_joins_n(bad.data(), lengths.data(), n, I, L, clamp, &byte, 1) == PF_EINVAL, "a slot outside [0, n)", "joins");
    }

    // supports of the tree among two replicates of itself: 100 after every inner node
    std::vector<float> reps(2 * P);
    memcpy(reps.data(), p, P * sizeof(float));
    memcpy(reps.data() + P, p, P * sizeof(float));
    const std::string sup = sized("support", [&](char* out, int64_t cap) { return pf_nj_support_n(p, reps.data(), 2, n, I, L, clamp, 2, out, cap); });
    expect(pf_nj_support_n(p, reps.data(), 0, n, I, L, clamp, 1, &byte, 1) == PF_EINVAL, "R = 0", "support");
    expect(pf_nj_support_n(p, nullptr, 2, n, I, L, clamp, 1, &byte, 1) == PF_EINVAL, "null reps", "support");
    expect(pf_nj_support_n(nullptr, reps.data(), 2, n, I, L, clamp, 1, &byte, 1) == PF_EINVAL, "null preds", "support");
    expect(pf_nj_support_n(p, reps.data(), 2, n, I, neg.data(), clamp, 1, &byte, 1) == PF_EINVAL, "a negative id length", "support");
    expect(pf_nj_support_n(p, reps.data(), 2, 0, I, L, clamp, 1, &byte, 1) == PF_EINVAL, "n = 0", "support");

    print_text("nj", 0, texts[0]);
    print_text("joins", 0, joined);
    print_text("bionj", 0, texts[1]);
    print_text("bme", steps[0], texts[2]);
    print_text("spr", steps[1], texts[3]);
    print_text("support", 0, sup);
    return misses ? 1 : 0;
}

template <class T>
void print_ints(const char* name, int flags, int branch, const std::vector<T>& v) {
    printf("%s %d %d:", name, flags, branch);
    for (const T x : v) printf(" %lld", (long long)x);
    printf("\n");
}

int supports_mode(int B, int R, int N, int cutoff, const char* path) {
    const size_t b = (size_t)B, r = (size_t)R, n = (size_t)N, T = 2 * (n - 3) + 3, S = n - 3;
    std::vector<int32_t> tables(b * T + b * r * T);
    std::vector<uint8_t> flag(b * r);
    {
        FILE* f = fopen(path, "rb");
        if (!f || fread(tables.data(), sizeof(int32_t), tables.size(), f) != tables.size() ||
            fread(flag.data(), 1, flag.size(), f) != flag.size())
            return 2;
        fclose(f);
    }
    const int32_t *ref = tables.data(), *rep = tables.data() + b * T;
    for (int flags = 0; flags < 2; ++flags) {
        const uint8_t* fl = flags ? flag.data() : nullptr;
        std::vector<int32_t> count(b * S, -1), depth(b * S, -1);
        std::vector<int64_t> transfer(b * S, -1);
        std::vector<uint8_t> status(b, 9);
        expect(pf_join_supports_host(ref, rep, fl, B, R, N, count.data(), transfer.data(), depth.data(), status.data()) == PF_OK, "PF_OK", "supports");
        print_ints("supports.count", flags, 0, count);
        print_ints("supports.transfer", flags, 0, transfer);
        print_ints("supports.depth", flags, 0, depth);
        print_ints("supports.status", flags, 0, status);
        for (int branch = 0; branch < 2; ++branch) {
            std::vector<int32_t> c2(b * S, -1), d2(b * S, -1), used(b * S, -1), capped(b * S, -1), moves_of(branch ? b * S * n : 0, -1);
            std::vector<int64_t> t2(b * S, -1), moves(b * n, -1);
            std::vector<uint8_t> s2(b, 9);
            expect(pf_join_transfers_host(ref, rep, fl, B, R, N, cutoff, c2.data(), t2.data(), d2.data(), moves.data(), used.data(),
                                          capped.data(), branch ? moves_of.data() : nullptr, s2.data()) == PF_OK, "PF_OK", "transfers");
            expect(c2 == count && t2 == transfer && d2 == depth && s2 == status, "the first three results are the supports'", "transfers");
            print_ints("transfers.moves", flags, branch, moves);
            print_ints("transfers.used", flags, branch, used);
            print_ints("transfers.capped", flags, branch, capped);
            if (branch) print_ints("transfers.branch_moves", flags, branch, moves_of);
        }
    }
    // each call's own refusals
    std::vector<int32_t> i32(b * S * n);
    std::vector<int64_t> i64(b * n > b * S ? b * n : b * S);
    std::vector<uint8_t> st(b);
    int32_t* x = i32.data();
    int64_t* y = i64.data();
    expect(pf_join_supports_host(ref, rep, nullptr, B, 0, N, x, y, x, st.data()) == PF_EINVAL, "R = 0", "supports");
    expect(pf_join_supports_host(ref, rep, nullptr, B, R, 3, x, y, x, st.data()) == PF_EINVAL, "N = 3", "supports");
    expect(pf_join_supports_host(ref, rep, nullptr, B, R, N, nullptr, y, x, st.data()) == PF_EINVAL, "null count", "supports");
    expect(pf_join_supports_host(rep, rep, nullptr, B, R, N, x, y, x, st.data()) == PF_OK, "a replicate as the reference", "supports");
    for (const int bad : {-1, 101})
        expect(pf_join_transfers_host(ref, rep, nullptr, B, R, N, bad, x, y, x, y, x, x, nullptr, st.data()) == PF_EINVAL, "a cutoff outside 0 .. 100", "transfers");
    expect(pf_join_transfers_host(ref, rep, nullptr, B, R, N, 50, x, y, x, nullptr, x, x, nullptr, st.data()) == PF_EINVAL, "null moves", "transfers");
    expect(pf_join_transfers_host(ref, rep, nullptr, B, R, N, 50, x, y, x, y, nullptr, x, nullptr, st.data()) == PF_EINVAL, "null used", "transfers");
    expect(pf_join_transfers_host(ref, rep, nullptr, B, R, N, 50, x, y, x, y, x, nullptr, nullptr, st.data()) == PF_EINVAL, "null capped", "transfers");
    expect(pf_join_transfers_host(ref, rep, nullptr, 0, R, N, 50, x, y, x, y, x, x, x, st.data()) == PF_EINVAL, "B = 0", "transfers");
    std::vector<int32_t> none(tables.begin(), tables.begin() + (std::ptrdiff_t)(b * T));
    std::fill(none.begin(), none.begin() + (std::ptrdiff_t)T, 0);
    expect(pf_join_supports_host(none.data(), rep, nullptr, B, R, N, x, y, x, st.data()) == PF_EINVAL, "a reference that is no join table", "supports");
    expect(pf_join_transfers_host(none.data(), rep, nullptr, B, R, N, 50, x, y, x, y, x, x, nullptr, st.data()) == PF_EINVAL,
           "a reference that is no join table", "transfers");
    return misses ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    int rc = 2;
    if (argc == 5 && !strcmp(argv[1], "text") && atoi(argv[2]) >= 3 && atoi(argv[2]) <= 4096)
        rc = text_mode(atoi(argv[2]), atoi(argv[3]), argv[4]);
    else if (argc == 7 && !strcmp(argv[1], "supports") && atoi(argv[2]) >= 1 && atoi(argv[3]) >= 1 && atoi(argv[4]) >= 4 && atoi(argv[4]) <= 4096)
        rc = supports_mode(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), argv[6]);
    if (rc == 0) printf("pf_hostio_trees_main: clean\n");
    return rc;
}
