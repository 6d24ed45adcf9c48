// device_owned.h -- the owners of everything the library takes from the HIP runtime: device allocations (through the guard bands), streams,
// events and the host-mapped status word.  An owner releases what it holds when it goes out of scope and cannot be copied; a struct that
// only READS another's buffers holds a plain pointer to that struct.  No hipFree, hipEventDestroy or hipStreamDestroy is written anywhere
// else.  Needs the HIP runtime API declared (hip/hip_runtime.h in the library; tests/asan/device_owned_host.cpp supplies counting stand-ins).
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <utility>
#include <vector>

// ---- guard bands (TCSFM_DEBUG_GUARDS=1; tcsfm_debug_check_guards): every device allocation of this library gets 4 KB filled with a pattern
// in front of it and behind it; the check reads the bands back and reports the allocations whose bands were written to.  A kernel's
// out-of-bounds WRITE into neighbouring scratch corrupts results silently (ADVICE r04 #1 went unnoticed for a round: hipMalloc's granularity
// hid it) and GPU AddressSanitizer is not available on this pool: the GPU test suite runs with the bands on instead (tests/conftest.py).
// Off (the default) the two functions are hipMalloc / hipFree themselves.
namespace tcguard {
constexpr size_t kBand = 4096;
constexpr unsigned char kFill = 0xA5;
struct Rec { char *base; size_t bytes; const char *file; int line; bool reported; };      // file: the call site's __FILE__
inline const char *at_file(const Rec &r) { const char *s = strrchr(r.file, '/'); return s ? s + 1 : r.file; }      // its base name, for the messages
inline std::mutex &mtx() { static std::mutex m; return m; }
inline std::vector<Rec> &recs() { static std::vector<Rec> r; return r; }
inline bool on() { static const bool v = getenv("TCSFM_DEBUG_GUARDS") && atoi(getenv("TCSFM_DEBUG_GUARDS")) != 0; return v; }
inline hipError_t alloc(void **p, size_t bytes, const char *file, int line) {
    if (!on()) return hipMalloc(p, bytes);
    char *base = nullptr;
    const size_t padded = (bytes + 255) / 256 * 256;            // (the rear band starts at the next 256-byte boundary: the user pointer keeps hipMalloc's alignment)
    hipError_t e = hipMalloc((void **)&base, padded + 2 * kBand);
    if (e != hipSuccess) return e;
    e = hipMemset(base, kFill, kBand);
    if (e == hipSuccess) e = hipMemset(base + kBand + bytes, kFill, padded - bytes + kBand);
    if (e != hipSuccess) { (void)hipFree(base); return e; }
    std::lock_guard<std::mutex> lk(mtx());
    recs().push_back({base, bytes, file, line, false});
    *p = base + kBand;
    return hipSuccess;
}
// number of bytes of the two bands of r that no longer hold the pattern (device synchronised by the copies)
inline long damaged(const Rec &r, long *first_off) {
    const size_t padded = (r.bytes + 255) / 256 * 256, rear = padded - r.bytes + kBand;
    std::vector<unsigned char> host(kBand + rear);
    if (hipMemcpy(host.data(), r.base, kBand, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(host.data() + kBand, r.base + kBand + r.bytes, rear, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    long bad = 0;
    for (size_t i = 0; i < host.size(); i++)
        if (host[i] != kFill) { if (!bad && first_off) *first_off = i < kBand ? (long)i - (long)kBand : (long)(r.bytes + (i - kBand)); bad++; }
    return bad;
}
inline hipError_t release(void *p) {
    if (!on() || !p) return hipFree(p);
    std::lock_guard<std::mutex> lk(mtx());
    for (size_t i = 0; i < recs().size(); i++)
        if (recs()[i].base + kBand == (char *)p) {
            long off = 0;
            const long bad = recs()[i].reported ? 0 : damaged(recs()[i], &off);
            if (bad > 0) fprintf(stderr, "tcsfm guard: allocation of %zu bytes (%s:%d) freed with %ld band bytes overwritten, first at offset %ld\n", recs()[i].bytes, at_file(recs()[i]), recs()[i].line, bad, off);
            char *base = recs()[i].base;
            recs().erase(recs().begin() + i);
            return hipFree(base);
        }
    return hipFree(p);      // (not one of ours)
}
// how many of the live allocations `ps` have a damaged band (reported on stderr once each); -1: a copy failed; guards off: 0.  For an entry that
// frees its allocations before it returns: tcsfm_debug_check_guards sees live records only, and release() can only print
inline int damaged_among(const std::vector<void *> &ps) {
    if (!on()) return 0;
    std::lock_guard<std::mutex> lk(mtx());
    int bad_allocs = 0;
    for (void *p : ps)
        for (auto &r : recs())
            if (r.base + kBand == (char *)p) {
                long off = 0;
                const long bad = damaged(r, &off);
                if (bad < 0) return -1;
                if (bad > 0) {
                    bad_allocs++;
                    if (!r.reported)
                        fprintf(stderr, "tcsfm guard: allocation of %zu bytes (%s:%d): %ld band bytes overwritten, first at offset %ld of the allocation\n", r.bytes, tcguard::at_file(r), r.line, bad, off);
                    r.reported = true;
                }
            }
    return bad_allocs;
}
}  // namespace tcguard

// One grow-only device buffer: p holds cap elements (byte buffers are DevBuf<char>), and reads as its pointer wherever one is expected.
// reserve() -- through DEV_RESERVE / RESERVE, which hand the call site to the guard bands -- keeps a buffer that is large enough (captured
// graphs bake the pointers in); otherwise it frees it, leaves the buffer empty (so it stays after a failed allocation) and allocates n
// elements.  A fixed-size buffer is one that is reserved once.  Whoever may still be using the old buffer on a stream is the caller's to
// wait for.  Moving hands the allocation over and leaves the source empty.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { (void)release(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { (void)release(); }
    operator T *() const { return p; }
    hipError_t reserve(size_t n, const char *file, int line) {
        if (cap >= n) return hipSuccess;
        hipError_t e = release();
        if (e == hipSuccess) e = tcguard::alloc((void **)&p, n * sizeof(T), file, line);
        if (e == hipSuccess) cap = n;
        else p = nullptr;
        return e;
    }
    hipError_t release() {
        const hipError_t e = p ? tcguard::release(p) : hipSuccess;
        p = nullptr; cap = 0;
        return e;
    }
};
#define DEV_RESERVE(buf, n) (buf).reserve((n), __FILE__, __LINE__)

struct NoCopy {      // an owner is not copied
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// A stream / an event of the library's own, created on first use; reads as its HIP handle (null before create()).
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipError_t create_with_priority(int priority) { return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
};
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    hipError_t create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
};
// ... and a growing list of events (timing: the profile brackets' pool; the others order streams only)
struct Events : NoCopy {
    std::vector<hipEvent_t> v;
    ~Events() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
    size_t size() const { return v.size(); }
    hipEvent_t operator[](size_t i) const { return v[i]; }
    hipError_t grow(size_t n, bool timing = false) {      // to n events; the ones made before a failure stay
        while (v.size() < n) {
            hipEvent_t e = nullptr;
            if (hipError_t rc = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming)) return rc;
            v.push_back(e);
        }
        return hipSuccess;
    }
};

// Pinned host memory, n elements, made once.
template <class T>
struct PinnedBuf : NoCopy {
    T *p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    operator T *() const { return p; }
    hipError_t create(size_t n, unsigned flags) { return hipHostMalloc((void **)&p, n * sizeof(T), flags); }
};
// The host-mapped status word of the device-side guards: kernels raise it through `dev`, the host reads and clears it through `host`.
struct MappedWord {
    PinnedBuf<int> host;
    int *dev = nullptr;
    hipError_t create() {
        hipError_t e = host.create(1, hipHostMallocMapped);
        if (e == hipSuccess) { *host = 0; e = hipHostGetDevicePointer((void **)&dev, host, 0); }
        return e;
    }
};
