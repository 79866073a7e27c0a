// contents_stash_test.cpp -- the stashed half spectrum in the record of what a plan's buffers hold (randomfield_amd/csrc/rf_contents.h):
// one predicate, stash(), and one transition, stash_ready().  Checked: (1) a new plan has no stash; (2) stash_ready() sets it and leaves
// every other predicate as it was, from every state the other transitions can reach; (3) no other transition changes it, in either
// value -- the stash is the caller's data and goes stale only with the plan; (4) the transition sequences of rf_kspace_stash,
// rf_kspace_interlace and rf_particles_paint_interlaced end where include/randomfield_hip.h says they do.  Stand-alone: compiled with
// -fsanitize=address,undefined and run by tests/test_contents_stash.py; exit status 0 = every check held.
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "../randomfield_amd/csrc/rf_contents.h"

namespace {

using rfc::Contents;

int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

char g_w, g_w2;
void* const W = &g_w;
void* const W2 = &g_w2;

// everything the predicates show but the stash
auto rest(const Contents& c) {
  return std::make_tuple(c.field(), c.where(), c.moments(), c.moments_pair(), c.kspace(), c.aux(), c.potential2(), c.counts(), c.deviates64(),
                         c.deviates32(), c.deviates());
}

struct Step {
  const char* name;
  void (*apply)(Contents&, void* buf, int pair);
};
// every transition of the record but stash_ready
const Step OTHERS[] = {
    {"field_ready", [](Contents& c, void* b, int s) { c.field_ready(b, s); }},
    {"field_written", [](Contents& c, void* b, int) { c.field_written(b); }},
    {"field_gathered", [](Contents& c, void* b, int) { c.field_gathered(b); }},
    {"field_modified", [](Contents& c, void*, int) { c.field_modified(); }},
    {"field_consumed", [](Contents& c, void*, int) { c.field_consumed(); }},
    {"not_a_field", [](Contents& c, void*, int) { c.not_a_field(); }},
    {"moments_ready", [](Contents& c, void*, int s) { c.moments_ready(s); }},
    {"moments_moved", [](Contents& c, void*, int s) { c.moments_moved(s); }},
    {"kspace_ready", [](Contents& c, void*, int) { c.kspace_ready(); }},
    {"kspace_consumed", [](Contents& c, void*, int) { c.kspace_consumed(); }},
    {"aux_ready", [](Contents& c, void*, int) { c.aux_ready(); }},
    {"kside_cleared", [](Contents& c, void*, int) { c.kside_cleared(); }},
    {"deviates_none", [](Contents& c, void*, int) { c.deviates_none(); }},
    {"deviates64_ready", [](Contents& c, void*, int) { c.deviates64_ready(); }},
    {"deviates32_ready", [](Contents& c, void*, int) { c.deviates32_ready(); }},
    {"deviates64_dropped", [](Contents& c, void*, int) { c.deviates64_dropped(); }},
    {"potential2_ready", [](Contents& c, void*, int) { c.potential2_ready(); }},
    {"potential2_stale", [](Contents& c, void*, int) { c.potential2_stale(); }},
    {"counts_ready", [](Contents& c, void*, int) { c.counts_ready(); }},
    {"counts_stale", [](Contents& c, void*, int) { c.counts_stale(); }},
};

// the states the other transitions reach from a new plan (buffers W / W2, pairs 0 / 1), by breadth-first search over what the predicates show
std::vector<Contents> reachable() {
  std::vector<Contents> states{Contents()};
  std::set<decltype(rest(Contents()))> seen{rest(Contents())};
  for (size_t i = 0; i < states.size(); ++i)
    for (const Step& st : OTHERS)
      for (void* buf : {W, W2})
        for (int pair : {0, 1}) {
          Contents c = states[i];
          st.apply(c, buf, pair);
          if (seen.insert(rest(c)).second) states.push_back(c);
        }
  return states;
}

}  // namespace

int main() {
  CHECK(!Contents().stash());
  const std::vector<Contents> states = reachable();
  CHECK(states.size() > 100);
  for (const Contents& s0 : states) {
    CHECK(!s0.stash());                                   // (2) nothing but stash_ready makes one ...
    Contents s1 = s0;
    s1.stash_ready();
    CHECK(s1.stash() && rest(s1) == rest(s0));            // ... and stash_ready touches nothing else
    Contents again = s1;
    again.stash_ready();
    CHECK(again.stash() && rest(again) == rest(s0));
    for (const Step& st : OTHERS)                         // (3) it survives every other transition, which does what it did without one
      for (void* buf : {W, W2})
        for (int pair : {0, 1}) {
          Contents with = s1, without = s0;
          st.apply(with, buf, pair);
          st.apply(without, buf, pair);
          CHECK(with.stash() && !without.stash() && rest(with) == rest(without));
        }
  }
  {   // rf_upload_k, rf_kspace_stash, rf_upload_k, rf_kspace_interlace: K stays k-space data, the stash stays
    Contents c;
    c.kspace_ready();
    CHECK(c.kspace() && !c.stash());
    c.stash_ready();
    c.kspace_ready();
    CHECK(c.kspace() && c.stash());
  }
  {   // rf_particles_paint_interlaced: paint, forward transform into the stash, shifted paint, forward transform, combine, c2r
    Contents c;
    c.counts_stale(); c.field_written(W); c.counts_ready();          // paint
    c.field_consumed();                                              // tiled forward passes in place; the spectrum goes to the stash:
    CHECK(!c.kspace());                                              // K and what it holds are as they were
    c.stash_ready();
    c.counts_stale(); c.field_written(W); c.counts_ready();          // shifted paint
    c.field_consumed(); c.kspace_ready();                            // forward transform into K
    CHECK(c.kspace() && c.stash() && !c.field());
    c.field_ready(W, 0);                                             // rf_execute_c2r
    CHECK(c.field_in(W) && c.moments() && c.kspace() && c.stash() && c.counts());
    c.kspace_consumed(); c.kside_cleared(); c.field_consumed(); c.counts_stale();      // whatever comes later: the stash is the caller's
    CHECK(c.stash());
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  if (g_failed == 0) std::printf("all checks passed\n");
  return g_failed ? 1 : 0;
}
