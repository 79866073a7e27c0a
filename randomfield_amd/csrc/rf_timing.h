// rf_timing.h -- what rf_elapsed_ms, rf_kernel_ms and rf_merged_yz_ms read: one call's start, its end, and the marks between them, each
// mark closing an interval that belongs to one of the five entries of rf_kernel_ms.  Every event read was recorded by the call that is
// read: begin() forgets the marks of the call before, and nothing is read until end() has closed this one.  The runtime is a template
// parameter as in rf_owned.h (rf_plan.h: HIP; tests/timing_test.cpp: a fake whose events carry a counter), so nothing here includes HIP.
#pragma once
#include <vector>

#include "rf_owned.h"

namespace rft {

enum Part { X = 0, Y = 1, Z = 2, REDUCE = 3, EXTRA = 4 };      // the entries of rf_kernel_ms

// Api: as rfo::EventList's, and Stream, not_ready (the answer of a timeline with nothing to read), event_record(Event, Stream),
// event_sync(Event), event_elapsed(float* ms, Event from, Event to)
template <class Api>
struct Timeline {
  using Error = typename Api::Error;
  using Event = typename Api::Event;
  struct Mark { Part part; bool merged; };
  rfo::EventList<Api> ev;              // [0] the start, [1] the end, [2 + i] mark i; grown on demand (flags 0: events that keep a time stamp)
  std::vector<Mark> marks;             // of the current call only
  bool detailed = false;               // the call takes marks (a timed realisation); else start and end alone (batches, transforms)
  bool complete = false;               // end() has closed the call; begin() clears it, so a call that fails half way leaves nothing to read
  bool spanning = false;               // a call made of timed calls is open (span_begin): their begin() keeps its start

  Error begin(typename Api::Stream s, bool detail) {
    complete = detailed = false;
    marks.clear();
    if (Error e = ev.ensure(2, 0); e != Api::ok) return e;
    detailed = detail;
    return spanning ? Api::ok : Api::event_record(ev[0], s);
  }
  // A call that is a sequence of timed calls (rf_particles_paint_interlaced): the start is recorded here and every begin() up to
  // span_end() leaves it alone, so rf_elapsed_ms covers the whole sequence.  span_end() closes it as a call without marks.
  Error span_begin(typename Api::Stream s) {
    spanning = false;
    if (Error e = begin(s, false); e != Api::ok) return e;
    spanning = true;
    return Api::ok;
  }
  Error span_end(typename Api::Stream s) {
    spanning = detailed = false;
    marks.clear();
    return end(s);
  }
  void span_abandon() { spanning = complete = false; }      // the sequence failed half way: nothing to read
  // detailed timelines only: what ran on s since the previous mark (or the start) belongs to `part`.  out: the mark's event, for a
  // launcher that records it AGAIN further on (the split generation pass, between its two launches): that moves the boundary later,
  // and never past the next mark, which is recorded after the launcher has returned.
  Error mark(Part part, typename Api::Stream s, Event* out = nullptr, bool merged = false) {
    if (!detailed) return Api::ok;
    if (Error e = ev.ensure(marks.size() + 3, 0); e != Api::ok) return e;
    const Event m = ev[marks.size() + 2];
    if (Error e = Api::event_record(m, s); e != Api::ok) return e;
    marks.push_back(Mark{part, merged});
    if (out) *out = m;
    return Api::ok;
  }
  // what lies between the last mark and here belongs to REDUCE.  (Again, behind work appended to a complete call: the end moves later.)
  Error end(typename Api::Stream s) {
    if (ev.size() < 2) return Api::not_ready;
    const Error e = Api::event_record(ev[1], s);
    complete = e == Api::ok;
    return e;
  }
  Error elapsed(float* ms) const {
    if (!complete) return Api::not_ready;
    if (Error e = Api::event_sync(ev[1]); e != Api::ok) return e;
    return Api::event_elapsed(ms, ev[0], ev[1]);
  }
  // per part the sum of its intervals, exactly 0 for a part without one; the intervals marked `merged`: their sum and number
  Error report(float ms5[5], float* merged_ms = nullptr, int* merged_count = nullptr) const {
    if (!complete || !detailed) return Api::not_ready;
    if (Error e = Api::event_sync(ev[1]); e != Api::ok) return e;
    float sum[5] = {0, 0, 0, 0, 0}, msum = 0, t = 0;
    int n = 0;
    for (size_t i = 0; i <= marks.size(); ++i) {
      const bool last = i == marks.size();
      if (Error e = Api::event_elapsed(&t, i ? ev[i + 1] : ev[0], last ? ev[1] : ev[i + 2]); e != Api::ok) return e;
      sum[last ? REDUCE : marks[i].part] += t;
      if (!last && marks[i].merged) { msum += t; ++n; }
    }
    for (int i = 0; i < 5; ++i) ms5[i] = sum[i];
    if (merged_ms) *merged_ms = msum;
    if (merged_count) *merged_count = n;
    return Api::ok;
  }
  Error merged(float* sum_ms, int* count) const { float ms5[5]; return report(ms5, sum_ms, count); }
};

}  // namespace rft
