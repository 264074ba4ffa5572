// Host-only test of the call scaffold in points2surf_amd/csrc/p2s_devcall.h: a counting fake of the block cache and of the few
// runtime calls the header makes stands in for the device, and records the ORDER of drains, frees and error texts, so the
// program runs anywhere (under the address and undefined-behaviour sanitizers: test_devcall_host.py).
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
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
constexpr hipError_t hipSuccess = 0, hipErrorLaunchFailure = 719;
typedef struct FakeStream *hipStream_t;
enum hipMemcpyKind { hipMemcpyDeviceToHost = 2 };
enum { P2S_OK = 0, P2S_EHIP = -2, P2S_ENOMEM = -3, P2S_ENODEVICE = -5 };
constexpr int P2S_MAX_DEVICES = 16;

struct Fake {
    std::map<void *, size_t> live;          // block -> bytes asked for
    std::vector<std::string> log;           // "sync", "alloc", "free", "error", "set_device", in call order
    std::vector<size_t> asked;              // bytes of every request, failed ones included
    std::string error;                      // the last error text
    int allocs = 0, fail_alloc = 0;         // request number fail_alloc (1-based) fails; 0: none
    int frees = 0, syncs = 0;
    int devices = 2, current = -1;
    hipError_t next_error = hipSuccess;     // what the next hipGetLastError returns
    std::vector<int> changed;               // what the device "writes" to ctl[0] round by round; past its end: 0
    size_t round = 0;
    hipStream_t stream = (hipStream_t)0x10;
    void restart() {
        CHECK(live.empty());
        *this = Fake();
    }
    size_t first(const char *what) const {
        for (size_t i = 0; i < log.size(); ++i)
            if (log[i] == what) return i;
        return log.size();
    }
    size_t count(const char *what) const {
        size_t n = 0;
        for (const std::string &l : log) n += l == what;
        return n;
    }
} g;

void *p2s_pool_alloc(int device, size_t bytes) {
    CHECK(device == 1 && bytes > 0);
    g.log.push_back("alloc");
    g.asked.push_back(bytes);
    if (++g.allocs == g.fail_alloc) return nullptr;
    void *p = malloc(bytes);
    CHECK(p);
    g.live[p] = bytes;
    return p;
}
void p2s_pool_free(int device, void *p) {
    CHECK(device == 1 && g.live.erase(p) == 1);      // unknown or already returned: abort
    g.log.push_back("free");
    ++g.frees;
    free(p);
}
hipError_t hipStreamSynchronize(hipStream_t s) {
    CHECK(s == g.stream);
    g.log.push_back("sync");
    ++g.syncs;
    return hipSuccess;
}
void p2s_set_error(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g.error = buf;
    g.log.push_back("error");
}
const char *hipGetErrorString(hipError_t e) { return e == hipErrorLaunchFailure ? "launch failure" : "?"; }
hipError_t hipGetLastError() {
    const hipError_t e = g.next_error;
    g.next_error = hipSuccess;
    return e;
}
hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t) {
    memset(p, v, bytes);
    return hipSuccess;
}
// the read-back of ctl[0] behind a round: the fake device's verdict
hipError_t hipMemcpyAsync(void *dst, const void *, size_t bytes, hipMemcpyKind, hipStream_t) {
    CHECK(bytes == 4);
    const int v = g.round < g.changed.size() ? g.changed[g.round] : 0;
    ++g.round;
    memcpy(dst, &v, 4);
    return hipSuccess;
}
int p2s_device_count() { return g.devices; }
hipError_t hipSetDevice(int d) {
    g.current = d;
    g.log.push_back("set_device");
    return hipSuccess;
}
#define P2S_HIP_CHECK(expr)                  \
    do {                                     \
        if ((expr) != hipSuccess) return P2S_EHIP; \
    } while (0)

#include "../points2surf_amd/csrc/p2s_devcall.h"

// ---- the tests -------------------------------------------------------------------------------------------------------
static void scratch_returns_everything_once() {
    g.restart();
    {
        PoolScratch scr(1, g.stream);
        int *a = scr.get<int>(100);
        double *b = scr.get<double>(1000);
        char *c = scr.get<char>(0);                          // an empty request still asks for a block of 256 bytes
        CHECK(a && b && c && g.live.size() == 3 && scr.held.size() == 3);
        CHECK(g.asked == std::vector<size_t>({400, 8000, 256}));
        CHECK(g.live.at(c) == 256 && g.syncs == 0 && g.frees == 0);
        CHECK(scr.get<int>(1) && g.asked.back() == 256);     // below 256 bytes: 256
    }
    CHECK(g.live.empty() && g.frees == 4 && g.syncs == 1);  // every block exactly once (a second return aborts in the fake)
    CHECK(g.first("sync") < g.first("free"));                // drained before the first block goes back
    g.restart();
    {
        PoolScratch scr(1, g.stream);                        // nothing held: the drain still happens, nothing is returned
    }
    CHECK(g.syncs == 1 && g.frees == 0);
}

static void failed_allocation_holds_nothing() {
    g.restart();
    g.fail_alloc = 2;
    {
        PoolScratch scr(1, g.stream);
        CHECK(scr.get<float>(10) != nullptr);
        CHECK(scr.get<float>(20) == nullptr && scr.held.size() == 1 && g.live.size() == 1);
        CHECK(scr.get<float>(30) != nullptr && scr.held.size() == 2);
    }
    CHECK(g.live.empty() && g.frees == 2 && g.allocs == 3);
}

struct Layout {
    int *a;
    double *b;
    char *absent;
    short *c;
    char *base;
    size_t bytes;
};
static Layout layout(char *base) {
    Carver c{base};
    Layout w;
    w.a = c.take<int>(3);                                    // 12 bytes -> 256
    w.b = c.take<double>(33);                                // 264 bytes -> 512
    w.absent = c.take<char>(1000, false);                    // absent: NULL, no room
    w.c = c.take<short>(128);                                // 256 bytes -> 256
    return c.done(w);
}
static void carve_and_carver() {
    const Layout size = layout(nullptr);                     // on a null base: the size, no pointers
    CHECK(size.base == nullptr && size.bytes == 1024 && !size.a && !size.b && !size.absent && !size.c);
    g.restart();
    {
        PoolScratch scr(1, g.stream);
        const Layout w = scr.carve(layout);
        CHECK(w.base && g.live.at(w.base) == 1024 && w.bytes == 1024 && scr.held.size() == 1);
        CHECK((char *)w.a == w.base && (char *)w.b == w.base + 256 && w.absent == nullptr && (char *)w.c == w.base + 768);
        memset(w.base, 0, w.bytes);                          // the whole layout lies inside the block (address sanitizer)
    }
    CHECK(g.live.empty());
    g.restart();
    g.fail_alloc = 1;
    {
        PoolScratch scr(1, g.stream);
        const Layout w = scr.carve(layout);                  // allocator failure: base == NULL, bytes = what was asked for
        CHECK(w.base == nullptr && w.bytes == 1024 && !w.a && scr.held.empty() && g.asked.back() == 1024);
    }
    CHECK(g.frees == 0);
}

static int checked_call(hipError_t e, PoolScratch &scr) {
    const hipStream_t s = scr.s;
    DEV_CHECK("unit", e);
    return P2S_OK;
}
static void check_macro_and_oom() {
    g.restart();
    {
        PoolScratch scr(1, g.stream);
        CHECK(scr.get<int>(1));
        CHECK(checked_call(hipSuccess, scr) == P2S_OK && g.syncs == 0 && g.error.empty());
        CHECK(checked_call(hipErrorLaunchFailure, scr) == P2S_EHIP);
        CHECK(g.error == "unit: launch failure (e)");
        CHECK(g.syncs == 1 && g.first("sync") < g.first("error") && g.frees == 0);     // drained, then the text; nothing freed yet
    }
    CHECK(g.syncs == 2 && g.first("error") < g.first("free"));
    g.restart();
    CHECK(dev_oom("unit", g.stream) == P2S_ENOMEM && g.error == "unit: out of device memory");
    CHECK(g.syncs == 1 && g.first("sync") < g.first("error"));
}

static void device_selection() {
    g.restart();
    CHECK(select_device("unit", 1) == P2S_OK && g.current == 1 && g.error.empty());
    g.current = -1;
    CHECK(select_device("unit", 2) == P2S_ENODEVICE && g.error == "unit: no such device 2" && g.current == -1);
    CHECK(select_device("unit", -1) == P2S_ENODEVICE && g.error == "unit: no such device -1");
    CHECK(select_device("unit", 0, "no HIP device") == P2S_OK && g.current == 0);
    CHECK(select_device("unit", 7, "no HIP device") == P2S_ENODEVICE && g.error == "unit: no HIP device 7");
    g.devices = 64;
    CHECK(select_device("unit", P2S_MAX_DEVICES) == P2S_ENODEVICE && g.count("set_device") == 2);
}

static void rounds_until_unchanged() {
    int ctl[1] = {7};
    std::vector<long long> seen;
    auto round = [&](long long i) {
        CHECK(ctl[0] == 0);                                  // cleared before every round
        seen.push_back(i);
    };
    g.restart();
    g.changed = {1, 1, 0, 1};                                // rounds 0 and 1 merge something, round 2 nothing
    long long rounds = -1;
    CHECK(until_unchanged("unit", "the rounds", 10, ctl, g.stream, round, &rounds) == P2S_OK);
    CHECK(rounds == 3 && seen == std::vector<long long>({0, 1, 2}) && g.error.empty());     // stops after the first unchanged one
    g.restart();
    seen.clear();
    CHECK(until_unchanged("unit", "the rounds", 10, ctl, g.stream, round) == P2S_OK && seen.size() == 1);      // no count asked for
    g.restart();
    seen.clear();
    g.changed = {1, 1, 1, 1, 1};
    CHECK(until_unchanged("unit", "the rounds", 4, ctl, g.stream, round, &rounds) == P2S_EHIP);                // fails at max_rounds
    CHECK(rounds == 4 && seen.size() == 4 && g.error == "unit: internal error (the rounds did not converge in 4 rounds)");
    g.restart();
    seen.clear();
    g.changed = {1, 1, 1, 0};
    CHECK(until_unchanged("unit", "the rounds", 4, ctl, g.stream, round, &rounds) == P2S_OK && rounds == 4);   // the last one allowed
    g.restart();
    seen.clear();
    g.changed = {1, 1};
    g.next_error = hipErrorLaunchFailure;                    // a launch of round 0 failed: the call ends drained, with the text
    CHECK(until_unchanged("unit", "the rounds", 4, ctl, g.stream, round, &rounds) == P2S_EHIP && seen.size() == 1);
    CHECK(g.error == "unit: launch failure (hipGetLastError())" && g.first("sync") < g.first("error"));
}

int main() {
    CHECK(blocks(0) == 1 && blocks(1) == 1 && blocks(256) == 1 && blocks(257) == 2 && blocks(2048, 1024) == 2 && blocks(2049, 1024) == 3);
    CHECK(blocks(3ll << 32) == (3u << 24));
    scratch_returns_everything_once();
    failed_allocation_holds_nothing();
    carve_and_carver();
    check_macro_and_oom();
    device_selection();
    rounds_until_unchanged();
    CHECK(g.live.empty());
    puts("devcall host test ok");
    return 0;
}
