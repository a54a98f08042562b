// Lists of arrays and their visitors (DESIGN.md sections 20-22, 24).  What is carved from one device allocation - a
// tree search's state, a host entry point's staging, a pair of tables - is named once, by a list: it calls
// v(pointer, elements) for every array, and v.flags(B, {pointers}) for the one-byte flags of a tree state's source, which
// share one span of 8 bytes per source.  Every array starts a span of its own, a multiple of `align` bytes long (8; 256
// for the attention operator), so it is aligned for its type in whatever order the list names it.  The workspace of B
// sources of a tree state is B * Measure's figure for one: an array of x bytes per source takes up(B x, 8) <= B up(x, 8).
// The list of a call's arrays (a host entry point's staging) names both sides of each:
// v.in(staged, callers, elements, need) for what goes up, v.out(...) for what comes down.  The layout visitors see the
// staged side (Sides), Upload / Download copy between the two, Missing says whether a required pointer is null.
// Plain C++, no HIP: tests/native/pf_layout_main.cpp and pf_staging_main.cpp run the lists on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <memory>
#include <vector>

namespace pfspan {

inline size_t up(size_t x, size_t align) { return (x + align - 1) / align * align; }

// What a null pointer of the caller's means for an array.  REQUIRED: a refusal.  OPTIONAL: the array keeps its span,
// nothing is copied and the staged pointer is null too.  ABSENT: the call does without the array, whatever the caller's
// pointer - no elements, the staged pointer null.
enum Need { REQUIRED, OPTIONAL, ABSENT };

// in / out of a visitor V that lays arrays out by V::operator()(pointer, elements)
template <class V> struct Sides {
    template <class T> void in(const T*& p, const T* callers, size_t count, Need need = REQUIRED) { side(p, callers, count, need); }
    template <class T> void out(T*& p, T* callers, size_t count, Need need = REQUIRED) { side(p, callers, count, need); }
private:
    template <class T> void side(T*& p, const void* callers, size_t count, Need need) {
        (*static_cast<V*>(this))(p, need == ABSENT ? 0 : count);
        if (need == ABSENT || (need == OPTIONAL && !callers)) p = nullptr;
    }
};

// the bytes of the spans
struct Measure : Sides<Measure> {
    size_t bytes = 0, align = 8;
    template <class T> void operator()(T*&, size_t count) { bytes += up(count * sizeof(T), align); }
    void flags(size_t B, std::initializer_list<uint8_t**>) { bytes += 8 * B; }
};

// spans of a device workspace, one after the other from `at`
struct Carve : Sides<Carve> {
    char* at;
    size_t align;
    Carve(char* at, size_t align = 8) : at(at), align(align) {}
    template <class T> void operator()(T*& p, size_t count) { p = reinterpret_cast<T*>(at); at += up(count * sizeof(T), align); }
    void flags(size_t B, std::initializer_list<uint8_t**> list) {
        size_t i = 0;
        for (uint8_t** p : list) *p = reinterpret_cast<uint8_t*>(at) + B * i++;
        at += 8 * B;
    }
};

// The host's state: one zeroed, exactly sized allocation per array (flags included), so that a sanitizer build has its
// red zones around every one of them.
struct Allocate : Sides<Allocate> {
    std::vector<std::unique_ptr<unsigned char[]>> owned;
    template <class T> void operator()(T*& p, size_t count) {
        owned.emplace_back(new unsigned char[count * sizeof(T)]());
        p = reinterpret_cast<T*>(owned.back().get());
    }
    void flags(size_t B, std::initializer_list<uint8_t**> list) { for (uint8_t** p : list) (*this)(*p, B); }
};

// A call's list under a visitor that has operator() alone: the staging side of every array, no pointer made null.  The
// lists' forms without the caller's side (pfnj::staging_arrays(v, s, chunk, N), ...) go through it.
template <class V> struct StagingOnly {
    V& v;
    template <class T> void in(const T*& p, const T*, size_t count, Need need = REQUIRED) { v(p, need == ABSENT ? 0 : count); }
    template <class T> void out(T*& p, T*, size_t count, Need need = REQUIRED) { v(p, need == ABSENT ? 0 : count); }
};

// the bytes of list(v), and its arrays from `base` (aligned to `align`, that many bytes long)
template <class List> inline size_t measure(List&& list, size_t align = 8) { Measure m; m.align = align; list(m); return m.bytes; }
template <class List> inline void carve(char* base, List&& list, size_t align = 8) { Carve c{base, align}; list(c); }

// The copies of a staged call.  copy(to, from, bytes) returns 0 or an error of its own kind (hipMemcpyAsync on a stream;
// memcpy in a CPU program); after the first error nothing more is copied and `err` keeps it.
template <class Copy> struct Upload {         // every input whose caller's pointer is there
    Copy copy;
    int err = 0;
    template <class T> void in(const T*& p, const T* callers, size_t count, Need need = REQUIRED) {
        if (need != ABSENT && callers && !err) err = (int)copy(const_cast<T*>(p), callers, count * sizeof(T));
    }
    template <class T> void out(T*&, T*, size_t, Need = REQUIRED) {}
};
template <class Copy> struct Download {       // every result
    Copy copy;
    int err = 0;
    template <class T> void in(const T*&, const T*, size_t, Need = REQUIRED) {}
    template <class T> void out(T*& p, T* callers, size_t count, Need need = REQUIRED) {
        if (need != ABSENT && !err) err = (int)copy(callers, p, count * sizeof(T));
    }
};
template <class List, class Copy> inline int upload(List&& list, Copy copy) { Upload<Copy> u{copy}; list(u); return u.err; }
template <class List, class Copy> inline int download(List&& list, Copy copy) { Download<Copy> d{copy}; list(d); return d.err; }

// is a required pointer of the caller's null?
struct Missing {
    bool any = false;
    template <class T> void in(const T*&, const T* callers, size_t, Need need = REQUIRED) { any = any || (need == REQUIRED && !callers); }
    template <class T> void out(T*&, T* callers, size_t, Need need = REQUIRED) { any = any || (need == REQUIRED && !callers); }
};
template <class List> inline bool missing(List&& list) { Missing m; list(m); return m.any; }

// spans of floats, `stride` for each of nb sources (the taxon-axis analyses' sub-calls: TaxonCuts::carve in pf_lib.hip)
struct FloatSpan { float** p; size_t stride; };
template <class V> inline void float_spans(V& v, std::initializer_list<FloatSpan> spans, size_t nb) {
    for (const FloatSpan& s : spans) v(*s.p, nb * s.stride);
}

// The workspace of the softmax attention operator (pf_mha.hip.h: MhaArgs; Frag = its 16-byte operand fragment) for
// `rows` rows of C tokens in `ntiles` key tiles of 32; carved with align = 256.
template <class V, class Frag>
inline void mha_arrays(V& v, Frag*& qp, Frag*& kp, Frag*& vp, float*& att, size_t rows, size_t heads, size_t ntiles, size_t C, size_t E) {
    static_assert(sizeof(Frag) == 16, "an MFMA operand fragment is 16 bytes");
    v(qp, 2 * rows * heads * ntiles * 32 * 2);
    v(kp, 2 * rows * heads * ntiles * 32 * 2);
    v(vp, 2 * rows * heads * ntiles * 64);
    v(att, rows * C * E);
}

}  // namespace pfspan
