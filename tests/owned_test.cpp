// owned_test.cpp -- the owning types of randomfield_amd/csrc/rf_owned.h against a fake runtime that counts calls and fails on request.
// Stand-alone: compiled with -fsanitize=address,undefined and run by tests/test_owned_types.py; exit status 0 = every check held.
// The failure paths checked here are reached in the product only when the device is out of memory, which no GPU test may provoke.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>

#include "../randomfield_amd/csrc/rf_owned.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

// the fake runtime: real host memory behind it, so that a double free or a leak is also the sanitizer's finding
struct Fake {
  using Error = int;
  using Event = int*;
  using Stream = int*;
  static constexpr Error ok = 0;
  static constexpr bool device = true;
  static std::string log;               // 'a' alloc, 'f' free, 'A' failed alloc: the order of the calls
  static size_t last_alloc;
  static int fail_allocs;               // the next so many allocations fail
  static int fail_events;
  static int events_made, events_destroyed, streams_made, streams_destroyed;
  static Error alloc(void** q, size_t n) {
    if (fail_allocs > 0) { --fail_allocs; log += 'A'; return 2; }
    *q = std::malloc(n);
    last_alloc = n;
    log += 'a';
    return ok;
  }
  static Error free(void* q) { std::free(q); log += 'f'; return ok; }
  static Error event_create(Event* e, unsigned) {
    if (fail_events > 0) { --fail_events; return 3; }
    *e = new int(0);
    ++events_made;
    return ok;
  }
  static Error event_destroy(Event e) { CHECK(*e == 0); ++*e; delete e; ++events_destroyed; return ok; }      // (destroyed once)
  static Error stream_create(Stream* s, unsigned) { *s = new int(0); ++streams_made; return ok; }
  static Error stream_destroy(Stream s) { delete s; ++streams_destroyed; return ok; }
};
std::string Fake::log;
size_t Fake::last_alloc = 0;
int Fake::fail_allocs = 0, Fake::fail_events = 0;
int Fake::events_made = 0, Fake::events_destroyed = 0, Fake::streams_made = 0, Fake::streams_destroyed = 0;

struct Host : Fake { static constexpr bool device = false; };      // pinned host memory: not counted as device bytes

using Buf = rfo::Buffer<Fake, double>;
static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "a buffer has one owner");
static_assert(std::is_move_constructible<Buf>::value && std::is_move_assignable<Buf>::value, "... and can change it");
static_assert(!std::is_copy_constructible<rfo::EventList<Fake>>::value && !std::is_copy_constructible<rfo::Stream<Fake>>::value, "one owner");

size_t live_bytes() { return rfo::live().device_bytes; }

void test_reserve() {
  Buf b;
  CHECK(!b && b.ptr == nullptr && b.bytes == 0);
  Fake::log.clear();
  CHECK(b.reserve(100) == 0);                              // empty: allocates exactly `need`
  CHECK(Fake::log == "a" && Fake::last_alloc == 100 && b.ptr && b.bytes == 100 && live_bytes() == 100);
  CHECK((void*)b.get() == b.ptr);
  void* first = b.ptr;
  CHECK(b.reserve(100) == 0 && b.reserve(7) == 0 && b.reserve(0) == 0);      // smaller or equal: no call, same memory
  CHECK(Fake::log == "a" && b.ptr == first && b.bytes == 100);
  CHECK(b.reserve(101) == 0);                              // larger: ONE free, then ONE allocation
  CHECK(Fake::log == "afa" && Fake::last_alloc == 101 && b.bytes == 101 && live_bytes() == 101);
  Fake::fail_allocs = 1;                                   // a failing allocation: the error, and an empty buffer
  CHECK(b.reserve(500) == 2);
  CHECK(Fake::log == "afafA" && b.ptr == nullptr && b.bytes == 0 && live_bytes() == 0);
  CHECK(b.reserve(8) == 0);                                // ... which the next (small) request fills again
  CHECK(Fake::log == "afafAa" && b.ptr && b.bytes == 8 && live_bytes() == 8);
  CHECK(b.release() == 0 && b.release() == 0);             // twice is harmless
  CHECK(Fake::log == "afafAaf" && b.ptr == nullptr && b.bytes == 0 && live_bytes() == 0);
}

// two buffers that belong together (W2 / R2, the two pinned seed slots, mt_counts / mt_offsets), grown the way the plan grows them
int reserve_pair(Buf& a, Buf& b, size_t need) {
  if (int e = a.reserve(need)) return e;
  return b.reserve(need);
}
void test_pair() {
  Buf a, b;
  Fake::log.clear();
  Fake::fail_allocs = 0;
  CHECK(a.reserve(64) == 0);
  Fake::fail_allocs = 1;
  CHECK(b.reserve(64) == 2);                               // the second of the pair fails ...
  CHECK(a.ptr && a.bytes == 64 && !b && b.bytes == 0);     // ... the first is intact
  void* keep = a.ptr;
  CHECK(reserve_pair(a, b, 64) == 0);                      // the next call allocates only what is missing
  CHECK(Fake::log == "aAa" && a.ptr == keep && b.ptr && b.bytes == 64 && live_bytes() == 128);
}

void test_lifetime() {
  Fake::log.clear();
  {
    Buf a;
    CHECK(a.reserve(32) == 0);
    void* q = a.ptr;
    Buf b(std::move(a));                                   // move empties the source
    CHECK(a.ptr == nullptr && a.bytes == 0 && b.ptr == q && b.bytes == 32);
    Buf c;
    CHECK(c.reserve(16) == 0);
    c = std::move(b);                                      // move assignment frees what the target held
    CHECK(b.ptr == nullptr && b.bytes == 0 && c.ptr == q && c.bytes == 32 && live_bytes() == 32);
    CHECK(Fake::log == "aaf");
  }
  CHECK(Fake::log == "aaff" && live_bytes() == 0);         // destruction frees, once
  {
    rfo::Buffer<Host, char> pinned;                        // host memory is owned the same way and not counted as device bytes
    CHECK(pinned.reserve(24) == 0 && pinned.bytes == 24 && live_bytes() == 0);
  }
  CHECK(Fake::log == "aaffaf");
}

void test_events() {
  {
    rfo::EventList<Fake> ev;
    CHECK(ev.ensure(2, 0) == 0 && ev.size() == 2 && Fake::events_made == 2 && rfo::live().events == 2);
    int* e0 = ev[0];
    CHECK(ev.ensure(2, 0) == 0 && ev.ensure(1, 0) == 0 && Fake::events_made == 2);      // enough: nothing happens
    CHECK(ev.ensure(5, 0) == 0 && ev.size() == 5 && Fake::events_made == 5 && ev[0] == e0);      // incremental
    Fake::fail_events = 1;
    CHECK(ev.ensure(7, 0) == 3 && ev.size() == 5 && rfo::live().events == 5);      // a failure keeps what exists ...
    CHECK(ev.ensure(7, 0) == 0 && ev.size() == 7 && Fake::events_made == 7);      // ... and the next call completes the list
    CHECK(Fake::events_destroyed == 0);
  }
  CHECK(Fake::events_destroyed == 7 && rfo::live().events == 0);      // every event once (event_destroy checks "once")
}

void test_streams() {
  {
    rfo::Stream<Fake> s;
    CHECK(!s && s.create(0) == 0 && s && Fake::streams_made == 1 && rfo::live().streams == 1);
    int* h = s;
    CHECK(s.create(0) == 0 && Fake::streams_made == 1 && (int*)s == h);      // idempotent
    rfo::Stream<Fake> never;                               // a stream that was never created destroys nothing
  }
  CHECK(Fake::streams_destroyed == 1 && rfo::live().streams == 0);
}

}  // namespace

int main() {
  test_reserve();
  test_pair();
  test_lifetime();
  test_events();
  test_streams();
  CHECK(rfo::live().device_bytes == 0 && rfo::live().events == 0 && rfo::live().streams == 0);      // the live counters at exit
  std::printf(g_failed ? "%d checks failed\n" : "owned types: all checks passed\n", g_failed);
  return g_failed ? 1 : 0;
}
