// Stand-alone sanitizer program for the owners of csrc/device_owned.h (DevBuf, Stream, Event, Events, PinnedBuf, MappedWord).  Its own main,
// no Python, no GPU:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I tightly_coupled_sfm_amd/csrc tests/asan/device_owned_host.cpp -o device_owned_host && ./device_owned_host
//
// The header calls the HIP runtime by name and nothing else, so the program declares the handful of names it uses and defines them as
// counting stand-ins over malloc: every allocation, stream and event made is entered in a set, and destroying one that is not in the set
// (a second free) or leaving one in it (a leak) fails the run -- AddressSanitizer watches the same memory from below.  The guard bands are
// off (TCSFM_DEBUG_GUARDS unset): tcguard::alloc / release are the pass-through the library runs with by default.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef struct StandInStream *hipStream_t;
typedef struct StandInEvent *hipEvent_t;
constexpr unsigned hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipHostMallocMapped = 2, hipHostMallocDefault = 0;

static std::set<void *> live_dev, live_host, live_streams, live_events;
static int n_alloc = 0, n_free = 0, n_bad = 0, fail_next_alloc = 0;

static hipError_t make(std::set<void *> &live, void **p, size_t bytes) {
    *p = malloc(bytes ? bytes : 1);
    live.insert(*p);
    return hipSuccess;
}
static hipError_t drop(std::set<void *> &live, void *p, const char *what) {
    if (!live.erase(p)) { printf("FAILED: %s of something not live (a second release?)\n", what); n_bad++; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}
static hipError_t hipMalloc(void **p, size_t bytes) {
    if (fail_next_alloc) { fail_next_alloc--; *p = nullptr; return hipErrorOutOfMemory; }
    n_alloc++;
    return make(live_dev, p, bytes);
}
static hipError_t hipFree(void *p) { if (!p) return hipSuccess; n_free++; return drop(live_dev, p, "hipFree"); }
static hipError_t hipMemset(void *p, int v, size_t n) { memset(p, v, n); return hipSuccess; }
static hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
static hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return make(live_host, p, bytes); }
static hipError_t hipHostFree(void *p) { return drop(live_host, p, "hipHostFree"); }
static hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned) { *dev = host; return hipSuccess; }
static hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return make(live_streams, (void **)s, 1); }
static hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return make(live_streams, (void **)s, 1); }
static hipError_t hipStreamDestroy(hipStream_t s) { return drop(live_streams, s, "hipStreamDestroy"); }
static hipError_t hipEventCreate(hipEvent_t *e) { return make(live_events, (void **)e, 1); }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make(live_events, (void **)e, 1); }
static hipError_t hipEventDestroy(hipEvent_t e) { return drop(live_events, e, "hipEventDestroy"); }

#include "device_owned.h"
#include <vector>

static int bad = 0;
#define CHECK(cond, ...)                                                                             \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (bad++ < 20) { printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                            \
    } while (0)
static bool all_released() { return live_dev.empty() && live_host.empty() && live_streams.empty() && live_events.empty(); }

// the handle's staging slots: a vector of buffers that grows while its buffers are live
static void growing_vector() {
    const int a0 = n_alloc, f0 = n_free;
    std::vector<void *> seen;
    {
        std::vector<DevBuf<char>> stage;
        for (int i = 0; i < 9; i++) {
            stage.resize(i + 1);                        // (Staging::scratch: one more slot, the earlier ones move when the vector reallocates)
            CHECK(DEV_RESERVE(stage[i], 100 + i) == hipSuccess, "slot %d", i);
            seen.push_back(stage[i].p);
            for (int k = 0; k <= i; k++) {
                CHECK(stage[k].p == seen[k] && stage[k].cap == (size_t)(100 + k), "slot %d after growing to %d", k, i + 1);
                memset(stage[k].p, k, stage[k].cap);    // (still ours: AddressSanitizer would say otherwise)
            }
            CHECK(n_free == f0, "growing to %d slots freed something", i + 1);
        }
        CHECK(n_alloc - a0 == 9 && live_dev.size() == 9, "%d allocations, %zu live", n_alloc - a0, live_dev.size());
    }
    CHECK(n_free - f0 == 9 && live_dev.empty(), "%d frees, %zu live", n_free - f0, live_dev.size());
}

static void reserve_contract() {
    DevBuf<float> b;
    CHECK(!b && b.cap == 0, "a new buffer is empty");
    CHECK(DEV_RESERVE(b, 64) == hipSuccess && b.p && b.cap == 64, "first reserve");
    float *p0 = b.p;
    const int a0 = n_alloc;
    CHECK(DEV_RESERVE(b, 64) == hipSuccess && DEV_RESERVE(b, 1) == hipSuccess && DEV_RESERVE(b, 0) == hipSuccess, "sufficient reserves");
    CHECK(b.p == p0 && b.cap == 64 && n_alloc == a0, "a sufficient reserve keeps the pointer (captured graphs bake it in)");
    fail_next_alloc = 1;
    CHECK(DEV_RESERVE(b, 128) == hipErrorOutOfMemory, "the failure is reported");
    CHECK(b.p == nullptr && b.cap == 0 && live_dev.empty(), "after a failed reserve the buffer is empty and the old allocation is gone");
    CHECK(DEV_RESERVE(b, 16) == hipSuccess && b.p && b.cap == 16 && n_alloc == a0 + 1, "the next reserve allocates");
    CHECK(DEV_RESERVE(b, 32) == hipSuccess && b.cap == 32 && live_dev.size() == 1, "growing frees the smaller buffer");
}

static void moves() {
    const int f0 = n_free;
    DevBuf<int> a;
    CHECK(DEV_RESERVE(a, 8) == hipSuccess, "reserve");
    int *p = a.p;
    {
        DevBuf<int> b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 8, "move construction is exact");
        DevBuf<int> c;
        CHECK(DEV_RESERVE(c, 4) == hipSuccess, "reserve");
        c = std::move(b);                               // c's own buffer goes, b's comes over
        CHECK(n_free == f0 + 1 && b.p == nullptr && c.p == p && c.cap == 8, "move assignment");
        DevBuf<int> &same = c;
        c = std::move(same);
        CHECK(c.p == p && c.cap == 8, "self-assignment keeps the buffer");
        a = std::move(c);
    }                                                   // b, c: moved from -- they free nothing
    CHECK(n_free == f0 + 1 && a.p == p && live_dev.size() == 1, "moved-from buffers freed nothing");
    a = DevBuf<int>();                                  // (dn_train_free's idiom)
    CHECK(n_free == f0 + 2 && live_dev.empty(), "assigning an empty buffer releases");
}

// the networks' sharing: the primary owns the weights, a clone reads them through a plain pointer
struct Weights { DevBuf<float> w[3]; };
struct Net {
    Weights own;
    const Weights *w = &own;
    DevBuf<float> act;
};
static Net *make_net(const Net *primary) {
    Net *n = new Net();
    if (primary) n->w = primary->w;
    else for (auto &b : n->own.w) CHECK(DEV_RESERVE(b, 10) == hipSuccess, "weights");
    CHECK(DEV_RESERVE(n->act, 20) == hipSuccess, "activations");
    return n;
}
static void shared_weights() {
    // the library's order: clones first (tcsfm_posenet_destroy, tcsfm_depthnet's seq_clone member) ...
    {
        const int f0 = n_free;
        Net *p = make_net(nullptr), *c = make_net(p);
        CHECK(c->w == &p->own && c->w->w[2].p == p->own.w[2].p, "the clone reads the primary's weights");
        delete c;
        CHECK(n_free == f0 + 1 && live_dev.size() == 4, "a clone frees its activations and none of the weights");
        delete p;
        CHECK(n_free == f0 + 5 && live_dev.empty(), "the primary frees the rest, once");
    }
    // ... and the other way round: a clone must not touch what it only pointed to, whenever it goes
    {
        const int f0 = n_free;
        Net *p = make_net(nullptr), *c = make_net(p);
        delete p;
        CHECK(n_free == f0 + 4 && live_dev.size() == 1, "the primary frees its weights and activations");
        delete c;
        CHECK(n_free == f0 + 5 && live_dev.empty(), "the clone frees its activations only");
    }
}

static void streams_and_events() {
    {
        Stream s, t, never;
        Event e, none;
        Events ring, pool;
        MappedWord word;
        PinnedBuf<double> pinned;
        CHECK(!(hipStream_t)never && !(hipEvent_t)none && ring.size() == 0 && !word.host, "owners start empty");
        CHECK(s.create() == hipSuccess && t.create_with_priority(-1) == hipSuccess && e.create() == hipSuccess, "create");
        CHECK(ring.grow(5) == hipSuccess && ring.size() == 5 && ring.grow(3) == hipSuccess && ring.size() == 5, "a list of events grows only");
        CHECK(pool.grow(64, true) == hipSuccess && pool.grow(128, true) == hipSuccess && pool.size() == 128, "the profile pool");
        CHECK(word.create() == hipSuccess && word.host && word.dev && *word.host == 0, "the status word starts at 0");
        CHECK(pinned.create(12, hipHostMallocDefault) == hipSuccess && pinned.p, "pinned memory");
        CHECK(live_streams.size() == 2 && live_events.size() == 1 + 5 + 128 && live_host.size() == 2, "what is live");
        CHECK((hipStream_t)s && ring[4] && ring[0] != ring[4], "owners read as their handles");
    }
    CHECK(all_released() && n_bad == 0, "every stream, event and pinned buffer destroyed once");
}

int main() {
    growing_vector();
    reserve_contract();
    moves();
    shared_weights();
    streams_and_events();
    CHECK(all_released(), "something is still live at the end");
    CHECK(n_bad == 0, "%d releases of something not live", n_bad);
    CHECK(n_alloc == n_free, "%d allocations, %d frees", n_alloc, n_free);
    if (bad) { printf("device_owned_host FAILED: %d checks\n", bad); return 1; }
    printf("device_owned_host ok: %d allocations, each freed once\n", n_alloc);
    return 0;
}
