// hip_owned.h — move-only owners of what the host side holds on the GPU: device memory, pinned host memory, events, streams.
// Each converts to the raw handle, so launches, copies and pointer arithmetic read as with raw pointers, and releases what it holds
// in its destructor.  An owner never synchronises: what a regrow has to wait for (a stream, an event) is one line at the call site,
// before reserve().  After a failed allocation an owner is empty and its capacity is 0.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace hip_owned __attribute__((visibility("hidden"))) {  // no dynamic symbols: one instance of the counters in the library
// live resources of the process (mrs_debug_live_resources): touched where something is allocated or freed, never on a launch path
inline std::atomic<long long> live_dev{0}, live_pinned{0}, live_events{0}, live_streams{0};

template <class T> inline constexpr size_t elem_bytes = sizeof(T);
template <> inline constexpr size_t elem_bytes<void> = 1;  // DevBuf<void> / PinnedBuf<void> count bytes

template <class T> struct DevBuf {  // hipMalloc, or hipExtMallocWithFlags(kind) for kind != 0 (the peer window's memory kinds)
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) reset(), p = o.p, cap = o.cap, o.p = nullptr, o.cap = 0;
    return *this;
  }
  ~DevBuf() { reset(); }
  operator T*() const { return p; }
  T*     get() const { return p; }
  size_t capacity() const { return cap; }  // elements
  void   reset() {
    if (p) (void)hipFree(p), --live_dev;
    p = nullptr, cap = 0;
  }
  hipError_t alloc(size_t n, unsigned kind = 0) {
    reset();
    void*      q = nullptr;
    hipError_t e = kind ? hipExtMallocWithFlags(&q, elem_bytes<T> * n, kind) : hipMalloc(&q, elem_bytes<T> * n);
    if (e == hipSuccess && q) p = static_cast<T*>(q), cap = n, ++live_dev;
    return e;
  }
  hipError_t reserve(size_t n, unsigned kind = 0) { return n > cap ? alloc(n, kind) : hipSuccess; }  // frees, then allocates — only to grow

 private:
  T*     p   = nullptr;
  size_t cap = 0;
};

template <class T> struct PinnedBuf {  // hipHostMalloc(flags)
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) reset(), p = o.p, cap = o.cap, o.p = nullptr, o.cap = 0;
    return *this;
  }
  ~PinnedBuf() { reset(); }
  operator T*() const { return p; }
  T*     get() const { return p; }
  size_t capacity() const { return cap; }
  void   reset() {
    if (p) (void)hipHostFree(p), --live_pinned;
    p = nullptr, cap = 0;
  }
  hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
    reset();
    void*      q = nullptr;
    hipError_t e = hipHostMalloc(&q, elem_bytes<T> * n, flags);
    if (e == hipSuccess && q) p = static_cast<T*>(q), cap = n, ++live_pinned;
    return e;
  }
  hipError_t reserve(size_t n, unsigned flags = hipHostMallocDefault) { return n > cap ? alloc(n, flags) : hipSuccess; }

 private:
  T*     p   = nullptr;
  size_t cap = 0;
};

struct Event {
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) reset(), e = o.e, o.e = nullptr;
    return *this;
  }
  ~Event() { reset(); }
  operator hipEvent_t() const { return e; }
  hipEvent_t get() const { return e; }
  void       reset() {
    if (e) (void)hipEventDestroy(e), --live_events;
    e = nullptr;
  }
  hipError_t create(unsigned flags = hipEventDefault) {  // idempotent: an event that exists stays (the lazily created ones)
    if (e) return hipSuccess;
    hipError_t rc = hipEventCreateWithFlags(&e, flags);
    if (rc == hipSuccess) ++live_events; else e = nullptr;
    return rc;
  }

 private:
  hipEvent_t e = nullptr;
};

struct Stream {
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) reset(), s = o.s, o.s = nullptr;
    return *this;
  }
  ~Stream() { reset(); }
  operator hipStream_t() const { return s; }
  hipStream_t get() const { return s; }
  void        reset() {
    if (s) (void)hipStreamDestroy(s), --live_streams;
    s = nullptr;
  }
  hipError_t create(unsigned flags) { return reset(), made(hipStreamCreateWithFlags(&s, flags)); }
  hipError_t create_priority(unsigned flags, int priority) { return reset(), made(hipStreamCreateWithPriority(&s, flags, priority)); }
  hipError_t create_cu_mask(uint32_t words, const uint32_t* mask) { return reset(), made(hipExtStreamCreateWithCUMask(&s, words, mask)); }

 private:
  hipError_t made(hipError_t rc) {
    if (rc == hipSuccess) ++live_streams; else s = nullptr;
    return rc;
  }
  hipStream_t s = nullptr;
};
}  // namespace hip_owned
using hip_owned::DevBuf;
using hip_owned::Event;
using hip_owned::PinnedBuf;
using hip_owned::Stream;
