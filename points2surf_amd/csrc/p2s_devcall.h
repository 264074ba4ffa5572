// The host scaffold of one call that works on blocks of the device's cache (p2s_pool_alloc): the blocks it holds, the exit on
// a HIP error or on exhausted memory, the launch size, the device, the loop over the rounds of a union-find ("who
// owns device memory").  Included behind p2s_internal.h by the geometry units (prepare, normals, Poisson, mesh); like
// p2s_devmem.h it names only a few runtime calls, so tests/devcall_host_test.cpp includes it behind a fake of them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

inline unsigned blocks(long long n, int per = 256) { return (unsigned)std::max<long long>(1, (n + per - 1) / per); }

// A HIP error or exhausted memory ends the call.  The stream is drained BEFORE the error text is set and the call returns;
// `s` is the call's stream.
inline int dev_hip_error(const char *who, hipError_t e, const char *what, hipStream_t s) {
    (void)hipStreamSynchronize(s);
    p2s_set_error("%s: %s (%s)", who, hipGetErrorString(e), what);
    return P2S_EHIP;
}
inline int dev_oom(const char *who, hipStream_t s) {
    (void)hipStreamSynchronize(s);
    p2s_set_error("%s: out of device memory", who);
    return P2S_ENOMEM;
}
#define DEV_CHECK(who, expr)                                                     \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) return dev_hip_error(who, _e, #expr, s);           \
    } while (0)

// the device of a call that names one: in range, present, current.  `none` is the wording of the error (Poisson's differs)
inline int select_device(const char *who, int device, const char *none = "no such device") {
    if (p2s_device_count() <= device || device < 0 || device >= P2S_MAX_DEVICES) {
        p2s_set_error("%s: %s %d", who, none, device);
        return P2S_ENODEVICE;
    }
    P2S_HIP_CHECK(hipSetDevice(device));
    return P2S_OK;
}

// One workspace layout is one function over a Carver (as carve of p2s_forward.hip): run on a null base it gives the size,
// on the block the pointers.  The function returns a struct that ends in `char *base; size_t bytes;`.
struct Carver {
    char *base;
    size_t at = 0;
    template <class T> T *take(size_t count, bool present = true) {      // an absent region: NULL, no room
        T *p = base && present ? (T *)(base + at) : nullptr;
        at += present ? (count * sizeof(T) + 255) & ~(size_t)255 : 0;
        return p;
    }
    template <class W> W done(W w) const {                             // the layout, complete
        w.base = base;
        w.bytes = at;
        return w;
    }
};

// The blocks of the device's cache that one call holds.  They all return when the call ends, on every exit, and the stream
// is drained first: no block goes back to the cache under a running kernel.
struct PoolScratch {
    int device;
    hipStream_t s;
    std::vector<void *> held;
    PoolScratch(int d, hipStream_t st) : device(d), s(st) {}
    PoolScratch(const PoolScratch &) = delete;
    ~PoolScratch() {
        (void)hipStreamSynchronize(s);
        for (void *p : held) p2s_pool_free(device, p);
    }
    template <class T> T *get(size_t count) {                            // NULL: out of memory, nothing held
        void *p = p2s_pool_alloc(device, std::max<size_t>(count * sizeof(T), 256));
        if (p) held.push_back(p);
        return (T *)p;
    }
    // a block of the layout `layout(base)`; out of memory: base == NULL (and bytes = what was asked for)
    template <class Fn> auto carve(Fn layout) -> decltype(layout((char *)nullptr)) {
        const auto size = layout((char *)nullptr);
        char *p = get<char>(size.bytes);
        return p ? layout(p) : size;
    }
};

// Rounds of a union-find until one changes nothing: `round(i)` launches round i, and a kernel of it that merged two trees
// raises ctl[0].  Every round that changes something merges two trees, so it ends; max_rounds only guards the host loop, and
// reaching it with a change in the last round is an error.  *rounds_out: the rounds made, the unchanged one included.
template <class Round>
int until_unchanged(const char *who, const char *what, long long max_rounds, int *ctl, hipStream_t s, Round round,
                    long long *rounds_out = nullptr) {
    int changed = 1;
    long long it = 0;
    for (; it < max_rounds && changed; ++it) {
        DEV_CHECK(who, hipMemsetAsync(ctl, 0, 4, s));
        round(it);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, hipMemcpyAsync(&changed, ctl, 4, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
    }
    if (rounds_out) *rounds_out = it;
    if (changed) {
        p2s_set_error("%s: internal error (%s did not converge in %lld rounds)", who, what, it);
        return P2S_EHIP;
    }
    return P2S_OK;
}
