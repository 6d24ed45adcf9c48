// The buffer-overlap contract of include/tcsfm.h ("Overlapping arguments"), enforced in one place: an entry point names every array
// argument of the call with its extent in bytes and its role, blesses the pairs the contract honours, and asks for the first forbidden
// overlap.  Host pointer arithmetic only: no device call.  Up to kInline arrays -- every pose, dense and operator entry -- nothing is
// allocated; a call that names more (the parameter tables of the networks and of an optimiser step over a real network) pays two heap
// vectors and a sort per call, a known cost of the training step.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct ArgRanges {
    struct R { const char *name; int idx; uintptr_t lo, hi; bool out; };       // idx >= 0: element of a pointer array, printed name[idx]
    struct Bless { const char *out, *in; bool any; };
    static constexpr int kInline = 32, kBless = 8;
    R small[kInline];
    std::vector<R> more;
    int n = 0, nb = 0;
    Bless blessed[kBless];
    bool io_free = false;      // the call stages host arrays: inputs go up before the first launch, outputs come back after the last

    const R &at(int i) const { return i < kInline ? small[i] : more[(size_t)(i - kInline)]; }
    // NULL arguments and zero-length arrays take part in nothing
    void add(const char *name, int idx, const void *p, size_t bytes, bool out) {
        if (!p || !bytes) return;
        const R r{name, idx, (uintptr_t)p, (uintptr_t)p + bytes, out};
        if (n < kInline) small[n] = r; else more.push_back(r);
        n++;
    }
    void in(const char *name, const void *p, size_t bytes, int idx = -1) { add(name, idx, p, bytes, false); }
    void out(const char *name, const void *p, size_t bytes, int idx = -1) { add(name, idx, p, bytes, true); }
    // honoured: `out` at the base address of `in` ...
    void bless(const char *out, const char *in) { assert(nb < kBless); if (nb < kBless) blessed[nb++] = {out, in, false}; }
    // ... or overlapping it in any way
    void bless_any(const char *out, const char *in) { assert(nb < kBless); if (nb < kBless) blessed[nb++] = {out, in, true}; }

    bool honoured(const R &o, const R &i) const {
        for (int k = 0; k < nb; k++)
            if (!strcmp(blessed[k].out, o.name) && !strcmp(blessed[k].in, i.name) && (blessed[k].any || o.lo == i.lo)) return true;
        return false;
    }
    static std::string label(const R &r) {
        if (r.idx < 0) return r.name;
        char b[24];
        snprintf(b, sizeof(b), "[%d]", r.idx);
        return std::string(r.name) + b;
    }
    // whether the overlapping pair (x, y) is forbidden; on refusal the output is named first
    bool forbidden(const R &x, const R &y, const char *entry, std::string &msg) const {
        if (!x.out && !y.out) return false;                                    // two inputs may share memory
        const R &o = x.out ? x : y, &i = x.out ? y : x;
        if (!i.out && (io_free || honoured(o, i))) return false;
        msg = std::string(entry) + ": " + label(o) + " overlaps " + label(i);
        return true;
    }
    // a forbidden overlap as "<entry>: <out> overlaps <other>" (true), or nothing (false).  The ranges are walked in address order, so
    // that the parameter tables of the networks and the optimiser (a hundred disjoint tensors) cost n log n, not n^2.
    bool refused(const char *entry, std::string &msg) const {
        int small_idx[kInline];
        std::vector<int> big_idx;
        int *idx = small_idx;
        if (n > kInline) { big_idx.resize((size_t)n); idx = big_idx.data(); }
        for (int i = 0; i < n; i++) idx[i] = i;
        std::sort(idx, idx + n, [&](int a, int b) { return at(a).lo != at(b).lo ? at(a).lo < at(b).lo : a < b; });
        for (int i = 0; i < n; i++)
            for (int j = i + 1; j < n && at(idx[j]).lo < at(idx[i]).hi; j++) {
                const int a = idx[i] < idx[j] ? idx[i] : idx[j], b = idx[i] < idx[j] ? idx[j] : idx[i];      // (registration order)
                if (forbidden(at(a), at(b), entry, msg)) return true;
            }
        return false;
    }
    // whether two named arrays of the call overlap (the dense modes pick their output path by it)
    bool overlap(const char *a_name, const char *b_name) const {
        for (int a = 0; a < n; a++)
            for (int b = 0; b < n; b++)
                if (!strcmp(at(a).name, a_name) && !strcmp(at(b).name, b_name) && at(a).lo < at(b).hi && at(b).lo < at(a).hi) return true;
        return false;
    }
};
