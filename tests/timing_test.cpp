// timing_test.cpp -- the interval recorder of randomfield_amd/csrc/rf_timing.h against a fake runtime whose events carry the value of a
// counter: work(n) advances it, event_elapsed is the difference.  Every sequence of begin / mark / end the library issues is walked and
// report, merged and elapsed are compared with literal values (the clock is integral: exact comparisons).  Stand-alone: compiled with
// -fsanitize=address,undefined and run by tests/test_timing.py; exit status 0 = every check held.
#include <cstdio>
#include <cstring>

#include "../randomfield_amd/csrc/rf_timing.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

struct FakeEvent { long at = -1; int call = -1; };      // the clock and the number of the call (begin) that recorded it last
struct Fake {
  using Error = int;
  using Event = FakeEvent*;
  using Stream = int;
  static constexpr Error ok = 0, not_ready = 7;
  static long clock;
  static int call;                      // begins so far
  static int stale_reads;               // events read that the current call did not record
  static int fail_events, events_made, events_destroyed;
  static void work(long n) { clock += n; }
  static Error event_create(Event* e, unsigned) {
    if (fail_events > 0) { --fail_events; return 3; }
    *e = new FakeEvent();
    ++events_made;
    return ok;
  }
  static Error event_destroy(Event e) { delete e; ++events_destroyed; return ok; }
  static Error event_record(Event e, Stream) { e->at = clock; e->call = call; return ok; }
  static Error event_sync(Event e) { if (e->call != call) ++stale_reads; return ok; }
  static Error event_elapsed(float* ms, Event a, Event b) {
    if (a->call != call || b->call != call) ++stale_reads;
    *ms = (float)(b->at - a->at);
    return ok;
  }
};
long Fake::clock = 0;
int Fake::call = 0, Fake::stale_reads = 0, Fake::fail_events = 0, Fake::events_made = 0, Fake::events_destroyed = 0;

using TL = rft::Timeline<Fake>;
using rft::EXTRA; using rft::REDUCE; using rft::X; using rft::Y; using rft::Z;

int begin(TL& t, bool detailed) { ++Fake::call; return t.begin(0, detailed); }
// a launch of n ticks, then a mark
void run(TL& t, long n, rft::Part part, bool merged = false) { Fake::work(n); CHECK(t.mark(part, 0, nullptr, merged) == 0); }

// report == want, elapsed == their sum, merged == (msum, mcount)
void expect(const TL& t, float x, float y, float z, float r, float e, float msum = 0, int mcount = 0) {
  float ms[5] = {-1, -1, -1, -1, -1}, total = -1, sum = -1;
  int n = -1;
  CHECK(t.report(ms) == 0 && t.elapsed(&total) == 0 && t.merged(&sum, &n) == 0);
  const float want[5] = {x, y, z, r, e};
  CHECK(std::memcmp(ms, want, sizeof(want)) == 0);
  CHECK(total == x + y + z + r + e);
  CHECK(sum == msum && n == mcount);
  if (std::memcmp(ms, want, sizeof(want)) != 0) std::printf("  got %g %g %g %g %g\n", ms[0], ms[1], ms[2], ms[3], ms[4]);
}

void test_whole_grid() {
  TL t;
  CHECK(begin(t, true) == 0);                       // tiled passes, exact generation: no EXTRA mark
  run(t, 10, X); run(t, 20, Y); run(t, 30, Z);
  Fake::work(4);                                    // the reduction
  CHECK(t.end(0) == 0);
  expect(t, 10, 20, 30, 4, 0);
  CHECK(begin(t, true) == 0);                       // fast generation: EXTRA in front of the pass, nothing between the start and it
  run(t, 0, EXTRA); run(t, 10, X); run(t, 20, Y); run(t, 30, Z);
  Fake::work(4);
  CHECK(t.end(0) == 0);
  expect(t, 10, 20, 30, 4, 0);
  CHECK(begin(t, true) == 0);                       // the split launcher records the EXTRA event again behind the kz = 0 tiles
  Fake::Event ev = nullptr;
  CHECK(t.mark(EXTRA, 0, &ev) == 0 && ev != nullptr);
  Fake::work(3);
  CHECK(Fake::event_record(ev, 0) == 0);
  run(t, 10, X); run(t, 20, Y); run(t, 30, Z);
  Fake::work(4);
  CHECK(t.end(0) == 0);
  expect(t, 10, 20, 30, 4, 3);
}

// y and z launches slab by slab, one launch per pass
void per_pass(TL& t, int nslab) {
  CHECK(begin(t, true) == 0);
  run(t, 0, EXTRA); run(t, 10, X);
  for (int i = 0; i < nslab; ++i) { run(t, 2 + i, Y); run(t, 5 + i, Z); }
  Fake::work(4);
  CHECK(t.end(0) == 0);
}
// ... and merged: y(0), a launch per slab but the last (z of slab i with y of slab i + 1), the last z
void merged(TL& t, int nslab) {
  CHECK(begin(t, true) == 0);
  run(t, 0, EXTRA); run(t, 10, X);
  run(t, 2, Y);
  for (int i = 0; i + 1 < nslab; ++i) run(t, 7 + i, Y, true);
  run(t, 5, Z);
  Fake::work(4);
  CHECK(t.end(0) == 0);
}
void test_slabs() {
  TL t;
  per_pass(t, 1); expect(t, 10, 2, 5, 4, 0);
  per_pass(t, 2); expect(t, 10, 2 + 3, 5 + 6, 4, 0);
  per_pass(t, 3); expect(t, 10, 2 + 3 + 4, 5 + 6 + 7, 4, 0);
  merged(t, 2); expect(t, 10, 2 + 7, 5, 4, 0, 7, 1);
  merged(t, 4); expect(t, 10, 2 + 7 + 8 + 9, 5, 4, 0, 7 + 8 + 9, 3);
  // a call with fewer marks than the one before reads none of that call's events
  Fake::stale_reads = 0;
  per_pass(t, 1);
  expect(t, 10, 2, 5, 4, 0);
  CHECK(Fake::stale_reads == 0);
  CHECK(t.marks.size() == 4 && t.ev.size() == 2 + 2 + 2 * 3);      // (the events of the three-slab call are kept, not read)
}

void test_other_schedules() {
  TL t;
  CHECK(begin(t, true) == 0);                       // exchange in sub-slabs: the whole forward half is X; then the gathering z pass, the all-reduce
  run(t, 50, X); run(t, 30, Z);
  Fake::work(6);
  CHECK(t.end(0) == 0);
  expect(t, 50, 0, 30, 6, 0);
  CHECK(begin(t, true) == 0);                       // generic plan, generation as a sweep of its own
  run(t, 9, EXTRA); run(t, 10, X); run(t, 20, Y); run(t, 30, Z);
  Fake::work(4);
  CHECK(t.end(0) == 0);
  expect(t, 10, 20, 30, 4, 9);
  CHECK(begin(t, true) == 0);                       // ... and generated inside the x pass
  run(t, 12, X); run(t, 20, Y); run(t, 30, Z);
  Fake::work(4);
  CHECK(t.end(0) == 0);
  expect(t, 12, 20, 30, 4, 0);
  CHECK(begin(t, true) == 0);                       // the paint: clear, scatter, convert; the call ends where the last launch ends
  run(t, 3, X); run(t, 40, Y); run(t, 5, Z);
  CHECK(t.end(0) == 0);
  expect(t, 3, 40, 5, 0, 0);
  CHECK(begin(t, true) == 0);                       // the gather: one part
  run(t, 17, X);
  CHECK(t.end(0) == 0);
  expect(t, 17, 0, 0, 0, 0);
}

void test_untimed_and_refusals() {
  TL t;
  float ms[5] = {-1, -1, -1, -1, -1}, total = -1, sum = -1;
  int n = -1;
  CHECK(t.elapsed(&total) == Fake::not_ready && t.report(ms) == Fake::not_ready && t.merged(&sum, &n) == Fake::not_ready);      // before any call
  CHECK(t.end(0) == Fake::not_ready && !t.complete);                                 // (an end without a begin is none)
  CHECK(begin(t, false) == 0);                      // a batch, a transform: start and end alone; marks are not taken
  const int made = Fake::events_made;
  Fake::work(8);
  CHECK(t.mark(X, 0) == 0 && t.marks.empty() && Fake::events_made == made);
  Fake::work(8);
  CHECK(t.elapsed(&total) == Fake::not_ready);      // open
  CHECK(t.end(0) == 0);
  CHECK(t.elapsed(&total) == 0 && total == 16);
  CHECK(t.report(ms) == Fake::not_ready && t.merged(&sum, &n) == Fake::not_ready && ms[0] == -1 && n == -1);
  Fake::work(5);                                    // work appended to a finished call: ending it again moves the end
  CHECK(t.end(0) == 0 && t.elapsed(&total) == 0 && total == 21);
  CHECK(begin(t, true) == 0);                       // a timed call that fails half way leaves nothing to read
  run(t, 10, X);
  CHECK(t.report(ms) == Fake::not_ready && t.elapsed(&total) == Fake::not_ready && t.merged(&sum, &n) == Fake::not_ready);
  CHECK(begin(t, true) == 0);                       // ... and the next call reads its own events only
  Fake::stale_reads = 0;
  run(t, 1, X); run(t, 2, Y); run(t, 3, Z);
  CHECK(t.end(0) == 0);
  expect(t, 1, 2, 3, 0, 0);
  CHECK(Fake::stale_reads == 0);
}

void test_event_failures() {
  {
    TL t;
    Fake::fail_events = 1;
    CHECK(begin(t, true) == 3 && !t.complete && !t.detailed && t.marks.empty());      // no event for the start
    float total = -1;
    CHECK(t.elapsed(&total) == Fake::not_ready);
    CHECK(begin(t, true) == 0);
    run(t, 10, X);
    Fake::fail_events = 1;
    Fake::work(20);
    CHECK(t.mark(Y, 0) == 3 && t.marks.size() == 1 && !t.complete);                   // no event for a mark: no mark, and the call is over
    float ms[5];
    CHECK(t.report(ms) == Fake::not_ready);
    CHECK(begin(t, true) == 0);                     // the next call finds its events
    run(t, 10, X); run(t, 20, Y);
    CHECK(t.end(0) == 0);
    expect(t, 10, 20, 0, 0, 0);
  }
  CHECK(Fake::events_made == Fake::events_destroyed);
}

}  // namespace

int main() {
  test_whole_grid();
  test_slabs();
  test_other_schedules();
  test_untimed_and_refusals();
  test_event_failures();
  CHECK(Fake::events_made == Fake::events_destroyed && rfo::live().events == 0);
  std::printf(g_failed ? "%d checks failed\n" : "timing: all checks passed\n", g_failed);
  return g_failed ? 1 : 0;
}
