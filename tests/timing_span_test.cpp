// timing_span_test.cpp -- a call made of timed calls in the interval recorder of randomfield_amd/csrc/rf_timing.h (span_begin / span_end /
// span_abandon, behind rf_particles_paint_interlaced) against a fake runtime whose events carry the value of a counter.  Checked:
// elapsed() after span_end covers everything from span_begin, whatever begin / mark / end the calls inside issued; report() is refused
// after a span; an abandoned span leaves nothing to read; the next plain call is timed on its own again.  Stand-alone: compiled with
// -fsanitize=address,undefined and run by tests/test_timing_span.py; exit status 0 = every check held.
#include <cstdio>

#include "../randomfield_amd/csrc/rf_timing.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

struct FakeEvent { long at = -1; };
struct Fake {
  using Error = int;
  using Event = FakeEvent*;
  using Stream = int;
  static constexpr Error ok = 0, not_ready = 7;
  static long clock;
  static void work(long n) { clock += n; }
  static Error event_create(Event* e, unsigned) { *e = new FakeEvent(); return ok; }
  static Error event_destroy(Event e) { delete e; return ok; }
  static Error event_record(Event e, Stream) { e->at = clock; return ok; }
  static Error event_sync(Event) { return ok; }
  static Error event_elapsed(float* ms, Event a, Event b) { *ms = (float)(b->at - a->at); return ok; }
};
long Fake::clock = 0;

using TL = rft::Timeline<Fake>;

// a paint: a detailed call of three marks; a transform: a plain call
void paint(TL& t, long n) {
  CHECK(t.begin(0, true) == 0);
  Fake::work(1); CHECK(t.mark(rft::X, 0) == 0);
  Fake::work(n); CHECK(t.mark(rft::Y, 0) == 0);
  Fake::work(2); CHECK(t.mark(rft::Z, 0) == 0);
  CHECK(t.end(0) == 0);
}
void transform(TL& t, long n) {
  CHECK(t.begin(0, false) == 0);
  Fake::work(n);
  CHECK(t.end(0) == 0);
}

}  // namespace

int main() {
  TL t;
  float ms = -1, ms5[5];
  // a plain call first: timed on its own
  transform(t, 5);
  CHECK(t.elapsed(&ms) == 0 && ms == 5);
  Fake::work(100);                                    // (idle time between calls belongs to nobody)
  // the span: paint, transform, untimed work, paint, transform, a sweep, a detailed transform
  CHECK(t.span_begin(0) == 0);
  CHECK(!t.complete);
  paint(t, 10);
  CHECK(t.elapsed(&ms) == 0 && ms == 13);             // (inside the span a call's end reads from the span's start)
  transform(t, 7);
  Fake::work(3);
  paint(t, 20);
  transform(t, 7);
  Fake::work(4);
  paint(t, 6);
  CHECK(t.span_end(0) == 0);
  CHECK(t.complete && !t.detailed && !t.spanning);
  CHECK(t.elapsed(&ms) == 0 && ms == 13 + 7 + 3 + 23 + 7 + 4 + 9);
  CHECK(t.report(ms5) == Fake::not_ready);            // per-kernel times are not a span's
  // the next call is its own again, marks and all
  Fake::work(50);
  paint(t, 30);
  CHECK(t.elapsed(&ms) == 0 && ms == 33);
  CHECK(t.report(ms5) == 0 && ms5[0] == 1 && ms5[1] == 30 && ms5[2] == 2 && ms5[3] == 0 && ms5[4] == 0);
  // a span that fails half way leaves nothing to read, and the recorder works afterwards
  CHECK(t.span_begin(0) == 0);
  paint(t, 10);
  t.span_abandon();
  CHECK(!t.complete && !t.spanning && t.elapsed(&ms) == Fake::not_ready);
  transform(t, 9);
  CHECK(t.elapsed(&ms) == 0 && ms == 9);
  // span_begin inside an abandoned or finished span starts afresh
  CHECK(t.span_begin(0) == 0);
  Fake::work(2);
  CHECK(t.span_begin(0) == 0);
  Fake::work(3);
  CHECK(t.span_end(0) == 0 && t.elapsed(&ms) == 0 && ms == 3);
  if (g_failed == 0) std::printf("all checks passed\n");
  return g_failed ? 1 : 0;
}
