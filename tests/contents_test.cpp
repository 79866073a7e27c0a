// contents_test.cpp -- the record of what a plan's buffers hold (randomfield_amd/csrc/rf_contents.h) against the ten plan members it
// replaced: real_valid, cur, stats_valid, stats_slot, k_valid, aux_valid, p2_valid, pa_valid, noise_resident, noise32_resident.  TABLE
// below says, member by member, what the assignment sites of the code before the change did for each transition (copied from those
// sites, not from the header).  Checked: (1) from every state the transitions can reach, every transition leaves the ten members, as
// the predicates show them, as TABLE says; (2) the K allocation's and the deviates' three values exclude each other in every such state;
// (3) the transition sequences of the calls named in main() end where include/randomfield_hip.h and DESIGN.md say they do, the old
// members walking beside them.  Stand-alone: compiled with -fsanitize=address,undefined and run by tests/test_contents.py; exit
// status 0 = every check held.
#include <cstdio>
#include <cstring>
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

char g_w, g_w2;                                // two field buffers: only their addresses are used
void* const W = &g_w;
void* const W2 = &g_w2;

// the ten members of the plan before the change
struct Old {
  bool real_valid = false;
  void* cur = nullptr;
  bool stats_valid = false;
  int stats_slot = 0;
  bool k_valid = false, aux_valid = false, p2_valid = false, pa_valid = false, noise_resident = false, noise32_resident = false;
  auto tie() const { return std::tie(real_valid, cur, stats_valid, stats_slot, k_valid, aux_valid, p2_valid, pa_valid, noise_resident, noise32_resident); }
  bool operator==(const Old& o) const { return tie() == o.tie(); }
  bool operator<(const Old& o) const { return tie() < o.tie(); }
};
// ... as the predicates show them
Old seen(const Contents& c) {
  Old o;
  o.real_valid = c.field(); o.cur = c.where(); o.stats_valid = c.moments(); o.stats_slot = c.moments_pair();
  o.k_valid = c.kspace(); o.aux_valid = c.aux(); o.p2_valid = c.potential2(); o.pa_valid = c.counts();
  o.noise_resident = c.deviates64(); o.noise32_resident = c.deviates32();
  return o;
}

// what an assignment site did to one member: left it, cleared it, set it, or stored the call's buffer / pair
enum Act { keep, F, T, arg };
struct Row {
  const char* name;
  void (*apply)(Contents&, void* buf, int pair);
  Act real_valid, cur, stats_valid, stats_slot, k_valid, aux_valid, p2_valid, pa_valid, noise_resident, noise32_resident;
};
const Row TABLE[] = {
    // field_ready(p, slot): cur = W, stats_slot = slot, real_valid = stats_valid = true; batch_ready: the same with the buffer of the last turn
    {"field_ready", [](Contents& c, void* b, int s) { c.field_ready(b, s); }, T, arg, T, arg, keep, keep, keep, keep, keep, keep},
    // rf_upload_real, rf_particles_paint_ex, rf_lpt2_source: cur = W.ptr; real_valid = true; stats_valid = false
    {"field_written", [](Contents& c, void* b, int) { c.field_written(b); }, T, arg, F, keep, keep, keep, keep, keep, keep, keep},
    // queue_z_slab: cur = W; real_valid = true
    {"field_gathered", [](Contents& c, void* b, int) { c.field_gathered(b); }, T, arg, keep, keep, keep, keep, keep, keep, keep, keep},
    // rf_lognormal, rf_affine_z, the sweep of rf_realise_scaled_potential: stats_valid = false
    {"field_modified", [](Contents& c, void*, int) { c.field_modified(); }, keep, keep, F, keep, keep, keep, keep, keep, keep, keep},
    // queue_r2c_single, queue_r2c_slab_cols, rf_realise_batch_reference: real_valid = false; stats_valid = false
    {"field_consumed", [](Contents& c, void*, int) { c.field_consumed(); }, F, keep, F, keep, keep, keep, keep, keep, keep, keep},
    // queue_c2r (stand-in exchange, direct stand-in), batch_ready(real = false), RF_FLAG_EXCHANGE_CHUNKS, rf_slab_r2c_rows: real_valid = false
    {"not_a_field", [](Contents& c, void*, int) { c.not_a_field(); }, F, keep, keep, keep, keep, keep, keep, keep, keep, keep},
    // gather_and_reduce: stats_slot = 0; stats_valid = true
    {"moments_ready", [](Contents& c, void*, int s) { c.moments_ready(s); }, keep, keep, T, arg, keep, keep, keep, keep, keep, keep},
    // rf_slab_backward: stats_slot = 0
    {"moments_moved", [](Contents& c, void*, int s) { c.moments_moved(s); }, keep, keep, keep, arg, keep, keep, keep, keep, keep, keep},
    // kspace_ready(p): k_valid = true; aux_valid = false
    {"kspace_ready", [](Contents& c, void*, int) { c.kspace_ready(); }, keep, keep, keep, keep, T, F, keep, keep, keep, keep},
    // rf_realise_lognormal, rf_realise_batch_reference, execute_derivative_c2r(RF_GRAD_FROM_KSPACE): k_valid = false
    {"kspace_consumed", [](Contents& c, void*, int) { c.kspace_consumed(); }, keep, keep, keep, keep, F, keep, keep, keep, keep, keep},
    // rf_lensing_potential: k_valid = false; aux_valid = true
    {"aux_ready", [](Contents& c, void*, int) { c.aux_ready(); }, keep, keep, keep, keep, F, T, keep, keep, keep, keep},
    // rf_lpt2_source: k_valid = false; aux_valid = false
    {"kside_cleared", [](Contents& c, void*, int) { c.kside_cleared(); }, keep, keep, keep, keep, F, F, keep, keep, keep, keep},
    // rf_noise_mt19937_ex (before the replay is checked), rf_mt_share_begin, rf_realise_batch_reference: both false
    {"deviates_none", [](Contents& c, void*, int) { c.deviates_none(); }, keep, keep, keep, keep, keep, keep, keep, keep, F, F},
    // upload_noise, rf_mt_share_finish, rf_noise_mt19937_ex(single = 0): noise_resident = true; noise32_resident = false
    {"deviates64_ready", [](Contents& c, void*, int) { c.deviates64_ready(); }, keep, keep, keep, keep, keep, keep, keep, keep, T, F},
    // rf_noise_mt19937_ex(single = 1): noise_resident = false; noise32_resident = true
    {"deviates32_ready", [](Contents& c, void*, int) { c.deviates32_ready(); }, keep, keep, keep, keep, keep, keep, keep, keep, F, T},
    // ensure_noise, the buffer too small: noise_resident = false
    {"deviates64_dropped", [](Contents& c, void*, int) { c.deviates64_dropped(); }, keep, keep, keep, keep, keep, keep, keep, keep, F, keep},
    // rf_lpt2_potential: p2_valid = true
    {"potential2_ready", [](Contents& c, void*, int) { c.potential2_ready(); }, keep, keep, keep, keep, keep, keep, T, keep, keep, keep},
    // potential_forward, rf_save_potential, rf_lpt2_source: p2_valid = false
    {"potential2_stale", [](Contents& c, void*, int) { c.potential2_stale(); }, keep, keep, keep, keep, keep, keep, F, keep, keep, keep},
    // rf_particles_paint_ex: pa_valid = true behind the paint, false in front of it
    {"counts_ready", [](Contents& c, void*, int) { c.counts_ready(); }, keep, keep, keep, keep, keep, keep, keep, T, keep, keep},
    {"counts_stale", [](Contents& c, void*, int) { c.counts_stale(); }, keep, keep, keep, keep, keep, keep, keep, F, keep, keep},
};

void act(bool& m, Act a) { if (a == F) m = false; else if (a == T) m = true; }
Old after(Old o, const Row& r, void* buf, int pair) {
  act(o.real_valid, r.real_valid); act(o.stats_valid, r.stats_valid); act(o.k_valid, r.k_valid); act(o.aux_valid, r.aux_valid);
  act(o.p2_valid, r.p2_valid); act(o.pa_valid, r.pa_valid); act(o.noise_resident, r.noise_resident); act(o.noise32_resident, r.noise32_resident);
  if (r.cur == arg) o.cur = buf;
  if (r.stats_slot == arg) o.stats_slot = pair;
  return o;
}
const Row& row(const char* name) {
  for (const Row& r : TABLE) if (!std::strcmp(r.name, name)) return r;
  std::printf("FAILED: no transition %s\n", name);
  ++g_failed;
  return TABLE[0];
}

// (1) and (2): the closure of the fresh state under every transition, with both buffers and three pairs as arguments
void test_transitions_and_exclusivity() {
  std::set<Old> known;
  std::vector<Contents> todo{Contents()};
  known.insert(seen(todo[0]));
  CHECK(seen(Contents()) == Old());                                            // a fresh plan: nothing, no buffer, pair 0
  size_t steps = 0;
  while (!todo.empty()) {
    const Contents c = todo.back();
    todo.pop_back();
    const Old o = seen(c);
    CHECK(!(c.kspace() && c.aux()));
    CHECK(!(c.deviates64() && c.deviates32()) && c.deviates() == (c.deviates64() || c.deviates32()));
    CHECK(c.field_in(W) == (o.real_valid && o.cur == W) && c.field_in(W2) == (o.real_valid && o.cur == W2) && !c.field_in(nullptr));
    CHECK(c.field() == (o.real_valid && o.cur != nullptr));                    // (the spelling of the particle calls)
    for (const Row& r : TABLE)
      for (void* buf : {W, W2})
        for (int pair = 0; pair < 3; ++pair) {
          Contents n = c;
          r.apply(n, buf, pair);
          const Old want = after(o, r, buf, pair);
          ++steps;
          if (!(seen(n) == want)) { std::printf("FAILED: %s from a reachable state leaves other members than the old code\n", r.name); ++g_failed; }
          if (known.insert(seen(n)).second) todo.push_back(n);
        }
  }
  std::printf("contents: %zu reachable states, %zu transitions applied\n", known.size(), steps);
  // every combination the transitions can make: 2 (field) x 2 (moments) x 3 (pairs) x 3 (K) x 3 (deviates) x 2 x 2, once without a buffer
  // (no field yet) and twice with one
  CHECK(known.size() == 3 * 3 * 3 * 2 * 2 * 2 * (1 + 2 * 2));
}

// (3) a call as the sequence of its transitions; the old members walk beside the record and must agree after every step
struct Plan {
  Contents has;
  Old old;
  void go(const char* name, void* buf = nullptr, int pair = 0) {
    const Row& r = row(name);
    r.apply(has, buf, pair);
    old = after(old, r, buf, pair);
    agree();
  }
  void agree() { CHECK(seen(has) == old); }
  // the calls
  void realise(bool generic) { if (generic) go("kspace_ready"); go("field_ready", W, 0); }
  void realise_slab() { go("field_gathered", W); go("moments_ready", nullptr, 0); }      // queue_z_slab inside gather_and_reduce
  void upload_real() { go("field_written", W); }
  void r2c(bool generic, bool unpack = true) { if (!generic) go("field_consumed"); if (generic || unpack) go("kspace_ready"); }
  void execute_c2r() { go("field_ready", W, 0); }
  void hessian_c2r_from_potential(bool generic) { if (!generic) { go("kspace_ready"); execute_c2r(); } else go("field_ready", W, 0); }
  void lpt2_source(bool generic) {
    go("potential2_stale");
    for (int i = 0; i < 6; ++i) hessian_c2r_from_potential(generic);
    go("field_written", W);
    go("kside_cleared");
  }
};

void test_sequences() {
  for (const bool generic : {false, true}) {
    {
      Plan p;                                                  // rf_realise
      p.realise(generic);
      CHECK(p.has.field_in(W) && p.has.moments() && p.has.moments_pair() == 0 && p.has.kspace() == generic && !p.has.aux());
    }
    {
      Plan p;                                                  // rf_upload_real, rf_execute_r2c
      p.upload_real();
      CHECK(p.has.field_in(W) && !p.has.moments());
      p.r2c(generic);
      CHECK(p.has.field() == generic && !p.has.moments() && p.has.kspace());
    }
    {
      Plan p;                                                  // rf_measure_power from the field, an auxiliary field in the K allocation
      p.realise(generic);
      p.go("aux_ready");
      p.r2c(generic, false);
      if (generic) CHECK(p.has.field_in(W) && p.has.moments() && p.has.kspace() && !p.has.aux());       // field kept, k space ready
      else CHECK(!p.has.field() && !p.has.moments() && !p.has.kspace() && p.has.aux());                  // field consumed, K untouched
    }
    {
      Plan p;                                                  // rf_execute_gradient_c2r from k space: consumed on both kinds of plan
      p.go("kspace_ready");                                    // (rf_generate)
      if (!generic) { p.go("kspace_ready"); p.execute_c2r(); } else p.go("field_ready", W, 0);
      p.go("kspace_consumed");
      CHECK(p.has.field_in(W) && p.has.moments() && !p.has.kspace() && !p.has.aux());
    }
    {
      Plan p;                                                  // rf_lpt2_source, an auxiliary field and an older second-order potential there
      p.realise(generic);
      p.go("aux_ready");
      p.go("potential2_ready");
      p.lpt2_source(generic);
      CHECK(p.has.field_in(W) && !p.has.moments() && !p.has.kspace() && !p.has.aux() && !p.has.potential2());
      p.r2c(generic);                                          // rf_lpt2_potential: the source, rf_execute_r2c, the division
      p.go("potential2_ready");
      CHECK(p.has.field() == generic && !p.has.moments() && p.has.kspace() && p.has.potential2());
      p.go("potential2_stale");                                // rf_realise_potential / rf_save_potential
      CHECK(!p.has.potential2());
    }
  }
  {
    Plan p;                                                    // rf_lensing_potential, then rf_realise_lognormal: "k space consumed" spares the auxiliary field
    p.go("kspace_ready");
    p.realise(false);
    p.go("aux_ready");
    CHECK(p.has.aux() && !p.has.kspace());
    p.go("field_ready", W, 0);
    p.go("kspace_consumed");
    CHECK(p.has.field_in(W) && p.has.moments() && p.has.aux() && !p.has.kspace());
  }
  {
    Plan p;                                                    // rf_particles_paint_ex, twice
    for (int i = 0; i < 2; ++i) {
      p.go("counts_stale");
      CHECK(!p.has.counts());
      p.go("field_written", W);
      p.go("counts_ready");
      CHECK(p.has.field_in(W) && !p.has.moments() && p.has.counts());
    }
  }
  {
    Plan p;                                                    // rf_realise on the slab path, rf_realise_batch of two, of three, with a stand-in exchange
    p.realise_slab();
    CHECK(p.has.field_in(W) && p.has.moments() && p.has.moments_pair() == 0);
    p.go("field_gathered", W); p.go("field_gathered", W2); p.go("field_ready", W2, 1);
    CHECK(p.has.field() && !p.has.field_in(W) && p.has.field_in(W2) && p.has.where() == W2 && p.has.moments() && p.has.moments_pair() == 1);
    p.go("field_gathered", W); p.go("field_gathered", W2); p.go("field_gathered", W); p.go("field_ready", W, 2);
    CHECK(p.has.field_in(W) && p.has.moments_pair() == 2);
    p.go("field_gathered", W); p.go("field_gathered", W2); p.go("field_ready", W2, 1); p.go("not_a_field");
    CHECK(!p.has.field() && !p.has.field_in(W2) && p.has.where() == W2 && p.has.moments() && p.has.moments_pair() == 1);
    p.realise_slab();
    p.go("not_a_field");                                       // RF_FLAG_EXCHANGE_CHUNKS
    CHECK(!p.has.field() && p.has.moments());
    p.go("field_gathered", W); p.go("moments_moved", nullptr, 0);          // rf_slab_backward
    CHECK(p.has.field_in(W) && p.has.moments() && p.has.moments_pair() == 0);
  }
  {
    // rf_realise_batch_reference: the old code cleared both flags, then set and cleared noise32_resident ALONE -- the same thing with
    // noise_resident already false.  The old members take those literal assignments here, not the table's rows.
    for (const bool fails : {false, true}) {
      Plan p;
      p.go("kspace_ready");
      p.realise(false);
      p.go("deviates64_ready");
      p.go("deviates_none");
      p.go("field_consumed");
      for (int i = 0; i < 2; ++i) { p.has.deviates32_ready(); p.old.noise32_resident = true; p.agree(); CHECK(p.has.deviates32()); }
      if (fails) {
        p.has.deviates_none(); p.old.noise32_resident = false; p.agree();
        CHECK(!p.has.deviates() && !p.has.field() && !p.has.moments() && p.has.kspace());
      } else {
        p.has.deviates32_ready(); p.old.noise32_resident = true; p.agree();
        p.go("field_ready", W, 1);
        p.go("kspace_consumed");
        CHECK(p.has.deviates32() && !p.has.deviates64() && p.has.field_in(W) && p.has.moments_pair() == 1 && !p.has.kspace());
      }
    }
  }
  {
    Plan p;                                                    // ensure_noise: a growing noise buffer drops float64 deviates, never float32 ones
    p.go("deviates64_ready"); p.go("deviates64_dropped");
    CHECK(!p.has.deviates());
    p.go("deviates32_ready"); p.go("deviates64_dropped");
    CHECK(p.has.deviates32() && p.has.deviates());
    p.go("deviates64_ready");                                  // host deviates replace the float32 ones
    CHECK(p.has.deviates64() && !p.has.deviates32());
  }
  CHECK(Contents().where() == nullptr);                        // rf_device_ptr answers W while no field was ever made
}

}  // namespace

int main() {
  test_transitions_and_exclusivity();
  test_sequences();
  if (g_failed) std::printf("%d of %d checks failed\n", g_failed, g_checks);
  else std::printf("contents: all checks passed (%d)\n", g_checks);
  return g_failed ? 1 : 0;
}
