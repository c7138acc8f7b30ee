// device_alloc.hpp -- the one seam through which the library allocates and frees device and pinned host memory, creates and destroys
// streams and events, and the move-only owners built on it (host code only).
//   raw_alloc / raw_free   hipMalloc / hipHostMalloc and their frees: the only calls of them in csrc/.  Every block is counted in two
//                          process-wide atomic counters (live_bytes: several devices are driven from host threads, ngpu > 1), read
//                          through sepfwi_debug_live_bytes.
//   Buffer<T, Mem>         owns one block of n elements and books its bytes in the tally (a long long of its owner: a session's
//                          device_bytes_, the observed store's tiers) it was given.  ensure(n) is the grow-only operation: nothing within
//                          capacity, else free FIRST and allocate after -- contents are never kept, peak memory does not grow -- and a
//                          failed allocation leaves the buffer empty with capacity 0, so no length can outlive its block.
//   Handle<T, destroy>     the same for a stream or an event.
// With SEPFWI_POISON=1 in the environment every fresh device allocation of the library is filled with 0xFF bytes (a NaN in every
// float, -1 in every int) before it is handed out: a kernel that reads memory nothing has written yet then poisons its outputs
// instead of silently seeing whatever the allocator left there (zeros in a fresh process, stale data after a free).  GPU
// AddressSanitizer is not available on the target pool; this is the uninitialised-read check that is (scripts/gpu_poison.sh).
// The owners need nothing of HIP: a program that defines SEPFWI_ALLOC_EXTERNAL before including this header supplies raw_alloc and
// raw_free itself (tests/native/device_buffer_check.cpp).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace sepfwi {

enum class Mem { Device, Pinned };

struct LiveBytes {
    std::atomic<long long> device{0}, pinned{0};
};
inline LiveBytes &live_bytes() {
    static LiveBytes l;
    return l;
}

// `bytes` > 0 of device or pinned host memory; throws when there is none.  raw_free takes what raw_alloc gave.
#ifndef SEPFWI_ALLOC_EXTERNAL
inline
#endif
void *raw_alloc(Mem kind, size_t bytes);
#ifndef SEPFWI_ALLOC_EXTERNAL
inline
#endif
void raw_free(Mem kind, void *p) noexcept;

template <class T, Mem K = Mem::Device>
class Buffer {
  public:
    Buffer() = default;
    explicit Buffer(long long *tally) : tally_(tally) {}
    Buffer(long long *tally, size_t n) : tally_(tally) { ensure(n); }
    Buffer(Buffer &&o) noexcept : p_(o.p_), n_(o.n_), tally_(o.tally_) { o.p_ = nullptr, o.n_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept {  // (takes the source's tally with its block)
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_, tally_ = o.tally_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~Buffer() { reset(); }

    T *get() const { return p_; }
    size_t size() const { return n_; }  // elements
    explicit operator bool() const { return p_ != nullptr; }
    void ensure(size_t n) {
        if (n <= n_) return;
        reset();
        p_ = static_cast<T *>(raw_alloc(K, n * sizeof(T)));
        n_ = n;
        book((long long)(n * sizeof(T)));
    }
    void reset() {
        if (!p_) return;
        raw_free(K, p_);
        book(-(long long)(n_ * sizeof(T)));
        p_ = nullptr, n_ = 0;
    }

  private:
    void book(long long bytes) {
        if (tally_) *tally_ += bytes;
        (K == Mem::Device ? live_bytes().device : live_bytes().pinned) += bytes;
    }
    T *p_ = nullptr;
    size_t n_ = 0;
    long long *tally_ = nullptr;
};
template <class T> using DevBuf = Buffer<T, Mem::Device>;
template <class T> using PinBuf = Buffer<T, Mem::Pinned>;

template <class T, void (*Destroy)(T)>
class Handle {
  public:
    Handle() = default;
    explicit Handle(T h) : h_(h) {}
    Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = T{}; }
    Handle &operator=(Handle &&o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = T{};
        }
        return *this;
    }
    ~Handle() { reset(); }
    T get() const { return h_; }
    operator T() const { return h_; }
    void reset() {
        if (h_ != T{}) Destroy(h_);
        h_ = T{};
    }

  private:
    T h_{};
};

}  // namespace sepfwi

#ifndef SEPFWI_ALLOC_EXTERNAL
#include <hip/hip_runtime.h>

#include "hip_check.hpp"

namespace sepfwi {

inline bool poison_allocations() {
    static const bool on = [] {
        const char *e = std::getenv("SEPFWI_POISON");
        return e && std::strcmp(e, "0") != 0 && e[0] != '\0';
    }();
    return on;
}

inline void *raw_alloc(Mem kind, size_t bytes) {
    void *p = nullptr;
    if (kind == Mem::Pinned) {
        HIP_OK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        return p;
    }
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess && poison_allocations()) {
        e = hipMemset(p, 0xFF, bytes);
        // hipMemset on device memory does not block the host, and the session's streams are non-blocking ones that do not wait for
        // the null stream: without this the fill could land AFTER the first kernels that write the buffer
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) (void)hipFree(p);
    }
    HIP_OK(e);
    return p;
}

inline void raw_free(Mem kind, void *p) noexcept {
    if (kind == Mem::Pinned)
        (void)hipHostFree(p);
    else
        (void)hipFree(p);
}

inline void destroy_stream(hipStream_t s) { (void)hipStreamDestroy(s); }
inline void destroy_event(hipEvent_t e) { (void)hipEventDestroy(e); }
using Stream = Handle<hipStream_t, destroy_stream>;
using Event = Handle<hipEvent_t, destroy_event>;

inline Stream make_stream() {  // a non-blocking stream: it does not wait for the null stream
    hipStream_t s = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return Stream(s);
}
inline Event make_event(bool timing) {
    hipEvent_t e = nullptr;
    if (timing)
        HIP_OK(hipEventCreate(&e));
    else
        HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return Event(e);
}

}  // namespace sepfwi
#endif
