// rt_mem.h -- the host side's owning buffers: device memory (DevBuf), its
// pinned host twin (PinnedBuf) and the "size query, grow, real call" pair of
// the launches that take temporary storage (with_tmp).  Nothing here decides
// a size: every site passes the count it needs and the count to allocate when
// it must grow (growing frees, and hipFree waits for the device).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

// Device memory of cap() elements of T (bytes for DevBuf<void>), freed by the
// destructor.  Converts to T* where a kernel parameter or pointer arithmetic
// wants one.  Every point that gives the memory up -- the destructor, reset(),
// a growing grow() -- is one hipFree, also of an empty buffer (a no-op): how
// many calls a run makes does not depend on what happens to be allocated.
template <class T>
class DevBuf {
  static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void_v<T>, char, T>);
  T* p_ = nullptr;
  size_t cap_ = 0;

 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      if (p_) (void)hipFree(p_);
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~DevBuf() { (void)hipFree(p_); }
  friend void swap(DevBuf& a, DevBuf& b) noexcept {
    std::swap(a.p_, b.p_);
    std::swap(a.cap_, b.cap_);
  }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }
  bool holds(size_t n) const { return p_ && cap_ >= n; }

  void reset() {
    (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // n elements into an empty buffer (at least 16 bytes); empty on failure
  hipError_t alloc(size_t n) {
    if (p_) reset();
    const size_t bytes = n * kElem;
    hipError_t e = hipMalloc((void**)&p_, bytes ? bytes : 16);
    if (e != hipSuccess) p_ = nullptr;
    cap_ = e == hipSuccess ? n : 0;
    return e;
  }
  // holds `need` elements afterwards: as it is, or freed and allocated anew
  // with `n` (>= need: the site's headroom); empty on failure
  hipError_t grow(size_t need, size_t n) {
    if (holds(need)) return hipSuccess;
    reset();
    return alloc(n);
  }
  // takes over n elements somebody else allocated with hipMalloc
  void adopt(T* p, size_t n) {
    if (p_) reset();
    p_ = p, cap_ = n;
  }
};

// Pinned host memory of cap() elements of T (the read-backs' landing places).
template <class T>
class PinnedBuf {
  T* p_ = nullptr;
  size_t cap_ = 0;

 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  bool holds(size_t n) const { return p_ && cap_ >= n; }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  hipError_t grow(size_t need, size_t n) {
    if (holds(need)) return hipSuccess;
    reset();
    hipError_t e = hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) p_ = nullptr;
    cap_ = e == hipSuccess ? n : 0;
    return e;
  }
};

// need + 1/2 + `pad`: the headroom of the candidate lists' buffers (past a
// new camera's estimate, the last build's size + 1/4 + 4096: growing a buffer
// frees the old one, and hipFree waits for the device -- a whole frame's host
// lead lost mid-build)
static inline size_t half_more(size_t need, size_t pad) { return need + need / 2 + pad; }

// The scans' and sorts' temporary storage: never null once ensured
// (rt_cand_scan takes a null temp for a size query, also on its one-workgroup
// path, which needs none); headroom: a new camera's sort is a little longer
static inline hipError_t ensure_tmp(DevBuf<void>& tmp, size_t bytes) {
  if (bytes < 256) bytes = 256;
  return tmp.grow(bytes, half_more(bytes, 65536));
}

// A call that takes temporary storage, made twice: call(nullptr, &bytes) asks
// the size, `tmp` is grown to hold it, call(tmp, &bytes) runs with tmp's
// whole capacity (run = false: the size query and the growth only).
template <class Call>
static inline hipError_t with_tmp(DevBuf<void>& tmp, Call&& call, bool run = true) {
  size_t bytes = 0;
  hipError_t e = call((void*)nullptr, &bytes);
  if (e == hipSuccess) e = ensure_tmp(tmp, bytes);
  if (e != hipSuccess || !run) return e;
  bytes = tmp.cap();
  return call(tmp.get(), &bytes);
}
