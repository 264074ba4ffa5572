// Host-only test of the owners in points2surf_amd/csrc/p2s_devmem.h: a counting fake of the HIP calls they make stands in
// for the runtime, so the program runs anywhere (under the address and undefined-behaviour sanitizers: test_devmem_host.py).
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                             \
        }                                                                        \
    } while (0)

// ---- the fake --------------------------------------------------------------------------------------------------------
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
constexpr unsigned hipHostMallocDefault = 0, hipEventDefault = 0;
typedef struct FakeEvent *hipEvent_t;
typedef struct FakeStream *hipStream_t;

struct Fake {
    std::map<void *, size_t> live[2];       // [0] device, [1] pinned: block -> bytes
    std::vector<size_t> order;              // bytes of every successful allocation, in call order
    std::set<void *> events, streams;
    int calls = 0, fail_at = 0;             // allocation number fail_at (1-based) fails; 0: none
    int frees = 0;
    hipError_t sticky = hipSuccess;
    size_t blocks() const { return live[0].size() + live[1].size(); }
    void restart(int fail) { CHECK(blocks() == 0); order.clear(); calls = 0; frees = 0; fail_at = fail; sticky = hipSuccess; }
} g;

static hipError_t fake_alloc(int kind, void **p, size_t bytes) {
    CHECK(bytes > 0);                        // alloc(0) must not reach the allocator
    if (++g.calls == g.fail_at) {
        *p = nullptr;
        return g.sticky = hipErrorOutOfMemory;
    }
    *p = malloc(bytes);
    CHECK(*p);
    g.live[kind][*p] = bytes;
    g.order.push_back(bytes);
    return hipSuccess;
}
static hipError_t fake_free(int kind, void *p) {
    CHECK(g.live[kind].erase(p) == 1);       // unknown, of the other kind or already freed: abort
    ++g.frees;
    free(p);
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(0, p, bytes); }
hipError_t hipFree(void *p) { return fake_free(0, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) { CHECK(flags == hipHostMallocDefault); return fake_alloc(1, p, bytes); }
hipError_t hipHostFree(void *p) { return fake_free(1, p); }
hipError_t hipGetLastError() { return std::exchange(g.sticky, hipSuccess); }

template <class H> static hipError_t fake_create(std::set<void *> &all, H *h) {
    if (++g.calls == g.fail_at) return g.sticky = hipErrorOutOfMemory;
    *h = (H)malloc(1);
    all.insert(*h);
    return hipSuccess;
}
static hipError_t fake_destroy(std::set<void *> &all, void *h) {
    CHECK(all.erase(h) == 1);
    free(h);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return fake_create(g.events, e); }
hipError_t hipEventDestroy(hipEvent_t e) { return fake_destroy(g.events, e); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return fake_create(g.streams, s); }
hipError_t hipStreamDestroy(hipStream_t s) { return fake_destroy(g.streams, s); }

#include "../points2surf_amd/csrc/p2s_devmem.h"

// ---- the tests -------------------------------------------------------------------------------------------------------
template <class Buf> static void one_block(int kind, size_t elem) {
    g.restart(0);
    {
        Buf a;
        CHECK(!a && a.get() == nullptr);
        CHECK(a.alloc(10) && a && g.live[kind].at(a.get()) == 10 * elem);
    }
    CHECK(g.blocks() == 0 && g.frees == 1);                 // scope exit
    {
        Buf a;
        CHECK(a.alloc(3));
        a.reset();
        CHECK(!a && g.blocks() == 0 && g.frees == 2);       // reset()
        a.reset();                                          // again: nothing to free
        CHECK(a.alloc(4) && a.alloc(5));                    // alloc on a live buffer frees it first
        CHECK(g.blocks() == 1 && g.frees == 3 && g.live[kind].at(a.get()) == 5 * elem);
        Buf b;
        CHECK(b.alloc(6));
        void *const pa = a.get();
        b = std::move(a);                                   // move-assign over a live buffer
        CHECK(!a && a.get() == nullptr && b.get() == pa && g.blocks() == 1 && g.frees == 4);
        Buf c(std::move(b));                                // move-construct
        CHECK(!b && c.get() == pa && g.blocks() == 1);
        Buf &self = c;
        c = std::move(self);                                // self-move keeps the block
        CHECK(c.get() == pa && g.blocks() == 1);
    }
    CHECK(g.blocks() == 0 && g.frees == 5);                 // the moved-from buffers freed nothing
    {
        Buf a;
        const int calls = g.calls;
        CHECK(a.alloc(0) && !a && g.calls == calls);        // alloc(0): empty, success, no call to the allocator
        CHECK(a.alloc(7) && a.alloc(0) && !a && g.blocks() == 0);      // and it still frees what the buffer held
    }
    g.restart(1);
    {
        Buf a;
        CHECK(!a.alloc(8) && !a && g.sticky == hipSuccess && g.blocks() == 0);       // failure: empty, error cleared
    }
    CHECK(g.frees == 0);
}

static void alloc_all() {
    const size_t want[5] = {4 * sizeof(float), 3 * sizeof(int), 7, 2 * sizeof(double), 5 * sizeof(short)};
    for (int k = 0; k <= 5; ++k) {                          // k = 0: no failure
        g.restart(k);
        DevBuf<float> a;
        PinnedBuf<int> b;
        DevBuf<void> c;
        DevBuf<double> d;
        PinnedBuf<short> e;
        const bool ok = p2s_alloc_all(a, 4, b, 3, c, 7, d, 2, e, 5);
        CHECK(ok == (k == 0) && g.sticky == hipSuccess);
        if (k) {
            CHECK(!a && !b && !c && !d && !e && g.blocks() == 0 && g.calls == k && g.frees == k - 1);
            continue;
        }
        CHECK(g.blocks() == 5 && g.order == std::vector<size_t>(want, want + 5));
        CHECK(g.live[0].at(a.get()) == want[0] && g.live[1].at(b.get()) == want[1] && g.live[0].at(c.get()) == want[2] &&
              g.live[0].at(d.get()) == want[3] && g.live[1].at(e.get()) == want[4]);
    }
    CHECK(g.blocks() == 0);
    g.restart(0);                                           // a count of 0 in the middle: that buffer stays empty
    DevBuf<int> a, b, c;
    CHECK(p2s_alloc_all(a, 1, b, 0, c, 2) && a && !b && c && g.calls == 2);
}

template <class H, class Create> static void one_handle(std::set<void *> &all, Create create) {
    g.restart(0);
    {
        H a, b;
        CHECK(!a && create(a) && a && all.count(a.get()) == 1);
        CHECK(create(a) && all.size() == 1);                // create on a live handle destroys it first
        CHECK(create(b) && all.size() == 2);
        void *const pa = a.get();
        b = std::move(a);
        CHECK(!a && b.get() == pa && all.size() == 1);
        H c(std::move(b));
        CHECK(!b && c.get() == pa);
        c.reset();
        CHECK(!c && all.empty());
        CHECK(create(c));
    }
    CHECK(all.empty());
    g.restart(1);
    H a;
    CHECK(!create(a) && !a && g.sticky == hipSuccess);
}

int main() {
    one_block<DevBuf<float>>(0, sizeof(float));
    one_block<DevBuf<void>>(0, 1);
    one_block<PinnedBuf<double>>(1, sizeof(double));
    alloc_all();
    one_handle<DevEvent>(g.events, [](DevEvent &e) { return e.create(); });
    one_handle<DevStream>(g.streams, [](DevStream &s) { return s.create(0, -1); });
    CHECK(g.blocks() == 0 && g.events.empty() && g.streams.empty());
    puts("devmem host test ok");
    return 0;
}
