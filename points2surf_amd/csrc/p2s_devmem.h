// Move-only owners of what a handle or a call holds on the device: one hipMalloc block, one pinned host block, one event,
// one stream ("who owns device memory").  Included behind <hip/hip_runtime.h> (p2s_common.h includes it first).
// No growth policy in here: the reserve functions keep theirs.  Kernels and launch structs take .get().
#pragma once
#include <cstddef>
#include <utility>

template <class T> inline constexpr size_t p2s_elem_bytes = sizeof(T);
template <> inline constexpr size_t p2s_elem_bytes<void> = 1;       // DevBuf<void>: the count is in bytes

// alloc(count elements) frees what the buffer holds first; count == 0 leaves it empty and succeeds without a call to the
// allocator.  On failure the buffer is empty and the sticky HIP error is cleared.
template <class T> class DevBuf {
    T *p_ = nullptr;
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
        return *this;
    }
    ~DevBuf() { reset(); }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    bool alloc(size_t count) {
        reset();
        void *p = nullptr;
        if (count && hipMalloc(&p, count * p2s_elem_bytes<T>) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        p_ = static_cast<T *>(p);
        return true;
    }
};

// the same over pinned host memory
template <class T> class PinnedBuf {
    T *p_ = nullptr;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
    }
    bool alloc(size_t count) {
        reset();
        void *p = nullptr;
        if (count && hipHostMalloc(&p, count * p2s_elem_bytes<T>, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        p_ = static_cast<T *>(p);
        return true;
    }
};

// (buffer, count) pairs, allocated in the order given; true if all succeed, otherwise every buffer given is left empty
inline bool p2s_alloc_all() { return true; }
template <class Buf, class... Rest> bool p2s_alloc_all(Buf &b, size_t count, Rest &&...rest) {
    if (b.alloc(count) && p2s_alloc_all(rest...)) return true;
    b.reset();
    return false;
}

class DevEvent {
    hipEvent_t e_ = nullptr;
public:
    DevEvent() = default;
    DevEvent(DevEvent &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    DevEvent &operator=(DevEvent &&o) noexcept {
        if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); }
        return *this;
    }
    ~DevEvent() { reset(); }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    bool create(unsigned flags = hipEventDefault) {
        reset();
        if (hipEventCreateWithFlags(&e_, flags) == hipSuccess) return true;
        (void)hipGetLastError();
        e_ = nullptr;
        return false;
    }
};

class DevStream {
    hipStream_t s_ = nullptr;
public:
    DevStream() = default;
    DevStream(DevStream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    DevStream &operator=(DevStream &&o) noexcept {
        if (this != &o) { reset(); s_ = std::exchange(o.s_, nullptr); }
        return *this;
    }
    ~DevStream() { reset(); }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
    void reset() {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    bool create(unsigned flags, int priority) {
        reset();
        if (hipStreamCreateWithPriority(&s_, flags, priority) == hipSuccess) return true;
        (void)hipGetLastError();
        s_ = nullptr;
        return false;
    }
};
