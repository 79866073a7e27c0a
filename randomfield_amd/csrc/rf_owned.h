// rf_owned.h -- owning handles for what a plan allocates: buffers (device or pinned host), events, streams.  Each releases what it
// holds in its destructor, so rf_plan keeps no list of them.  The runtime is a template parameter (rf_plan.h: HIP; tests/owned_test.cpp:
// a fake that counts calls and fails on request), so nothing here includes HIP.
#pragma once
#include <atomic>
#include <cstddef>
#include <utility>
#include <vector>

namespace rfo {

// what the handles of this process hold right now (rf_diag_live_resources): device bytes, events, streams
struct Live {
  std::atomic<size_t> device_bytes{0};
  std::atomic<int> events{0}, streams{0};
};
inline Live& live() { static Live l; return l; }

struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};

// Alloc: Error, ok, device (counted in Live::device_bytes), alloc(void**, size_t), free(void*).  T: what get() points at.
template <class Alloc, class T = void>
struct Buffer : NoCopy {
  using Error = typename Alloc::Error;
  void* ptr = nullptr;
  size_t bytes = 0;
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) { (void)release(); ptr = std::exchange(o.ptr, nullptr); bytes = std::exchange(o.bytes, 0); }
    return *this;
  }
  ~Buffer() { (void)release(); }
  // room for `need` bytes.  Growing releases first, so that the peak is not old + new; after any failure the buffer is empty and the
  // next call tries again.
  Error reserve(size_t need) {
    if (bytes >= need) return Alloc::ok;
    if (Error e = release(); e != Alloc::ok) return e;
    void* q = nullptr;
    if (Error e = Alloc::alloc(&q, need); e != Alloc::ok) return e;
    ptr = q; bytes = need;
    if (Alloc::device) live().device_bytes += need;
    return Alloc::ok;
  }
  Error release() {
    if (!ptr) return Alloc::ok;
    if (Alloc::device) live().device_bytes -= bytes;
    bytes = 0;
    return Alloc::free(std::exchange(ptr, nullptr));
  }
  T* get() const { return static_cast<T*>(ptr); }
  explicit operator bool() const { return ptr != nullptr; }
};

// Api: Error, ok, Event, event_create(Event*, unsigned flags), event_destroy(Event)
template <class Api>
struct EventList : NoCopy {
  using Error = typename Api::Error;
  std::vector<typename Api::Event> ev;
  ~EventList() {
    for (auto e : ev) (void)Api::event_destroy(e);
    live().events -= (int)ev.size();
  }
  Error ensure(size_t n, unsigned flags) {       // grow to n events (flags as the runtime's create call takes them)
    while (ev.size() < n) {
      typename Api::Event e;
      if (Error r = Api::event_create(&e, flags); r != Api::ok) return r;
      ev.push_back(e);
      ++live().events;
    }
    return Api::ok;
  }
  size_t size() const { return ev.size(); }
  typename Api::Event operator[](size_t i) const { return ev[i]; }
};

// Api: Error, ok, Stream (a pointer-like handle), stream_create(Stream*, unsigned flags), stream_destroy(Stream)
template <class Api>
struct Stream : NoCopy {
  using Error = typename Api::Error;
  typename Api::Stream s{};
  ~Stream() {
    if (s) { (void)Api::stream_destroy(s); --live().streams; }
  }
  Error create(unsigned flags) {                 // idempotent
    if (s) return Api::ok;
    Error r = Api::stream_create(&s, flags);
    if (r == Api::ok) ++live().streams; else s = {};
    return r;
  }
  operator typename Api::Stream() const { return s; }
};

}  // namespace rfo
