// source_test.cpp -- which generator fills an x pass (randomfield_amd/csrc/rf_source.h) against the spellings it replaced.  The functions
// of namespace old below are LITERAL COPIES of the expressions the C-API layer worked the answer out with before the change (rf_capi.hip
// queue_x, potential_forward, rf_can_regenerate_potential, rf_diag_generation_path, rf_generate, the generic branch of queue_c2r;
// rf_capi_mt.hip rf_noise_mt19937_ex, rf_realise_batch_reference, rf_can_batch_reference), over structs that have the members they read.
// Every combination is walked: dtype x have_fast x exact_gen x the five route kinds x three deviate states x k-space given or not x
// three modes x three asks = 2160.  On every combination the entry points can reach, each old expression must equal the new answer --
// the branch taken, the buffers wired, whether refused, and the text; on the excluded ones source_of must still return a kind or a
// refusal.  Stand-alone: compiled with -fsanitize=address,undefined and run by tests/test_source.py; exit status 0 = every check held.
#include <cstdio>
#include <cstring>

#include "../randomfield_amd/csrc/rf_source.h"

namespace {

using rfc::Route;
using rfc::Source;
using rfc::SourceAsk;
using rfc::SourceFacts;

int g_failed = 0, g_checks = 0;
char g_where[200];
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) { std::printf("FAILED %s:%d: %s   [%s]\n", __FILE__, __LINE__, #cond, g_where); ++g_failed; } \
  } while (0)

// the refusals' texts, as the entry points print them
const char* const T_PAIRS_ONLY =
    "only float32 copies of the deviates are resident: this path (exact chain / float64 plan) needs rf_noise_mt19937's float64 ones";
const char* const T_REPLICATED = "replicated generation needs the native generator (fast path)";
const char* const T_GENERIC = "no float64 deviates resident on the device";
const char* const T_GENERATE = "rf_generate needs float64 deviates: only float32 copies are resident";
const char* const T_BESIDE = "this generation source cannot store or emit the potential";      // new: no entry point reaches it

// what the old expressions read: the plan's members of that name, `has` with the two predicates of rf_contents.h, route(p) with the
// two of rf_route.h, and the call's descriptor and generator parameters as they were
enum { RF_NOISE_NATIVE = 0, RF_NOISE_EXTERNAL = 1, RF_NOISE_RESIDENT = 2 };
enum { NOISE_PHILOX = 0, NOISE_EXTERNAL = 1 };
struct Has {
  bool d32, d64;
  bool deviates32() const { return d32; }
  bool deviates64() const { return d64; }
};
struct Plan {
  int f64;
  bool have_fast, exact_gen, generic, unpacked;
  Route::Kind kind;
  Has has;
};
Route route(const Plan* p) { Route r; r.kind = p->kind; return r; }
struct CallDesc { bool resident_fast = false, emit_potential = false; const void* pot_target = nullptr; };
struct GenParams { int noise_mode; };
// make_gen's line, and the six entry points' `cd.resident_fast = (mode == RF_NOISE_RESIDENT)`
GenParams make_gen(int mode) { return GenParams{(mode == RF_NOISE_RESIDENT) ? (int)RF_NOISE_EXTERNAL : mode}; }

namespace old {
// rf_capi.hip queue_x: the two refusals, the branch, and what it wired into the fast kernel's parameters
struct X { const char* refusal = nullptr; bool fast = false, noise32 = false, noise = false; };
X queue_x(const Plan* p, const CallDesc& cd, const GenParams& gp, const void* kspace) {
  X x;
  const bool rep = route(p).replicates();
  const bool fast_noise = !kspace && gp.noise_mode == NOISE_EXTERNAL && cd.resident_fast && p->have_fast && !p->exact_gen &&
                          !p->f64 && !rep && (p->has.deviates32() || !cd.pot_target);
  if (!(kspace || gp.noise_mode != NOISE_EXTERNAL || fast_noise || p->has.deviates64())) { x.refusal = T_PAIRS_ONLY; return x; }
  const bool fast = (!kspace && gp.noise_mode == NOISE_PHILOX && p->have_fast && !p->exact_gen) || fast_noise;
  if (!(!rep || fast)) { x.refusal = T_REPLICATED; return x; }
  if (fast_noise && p->has.deviates32()) x.noise32 = true;
  else if (fast_noise) x.noise = true;
  x.fast = fast;
  return x;
}
// rf_capi.hip potential_forward
bool fused(const Plan* p, int mode) {
  return ((mode == RF_NOISE_NATIVE) || (mode == RF_NOISE_RESIDENT && p->has.deviates32() && !p->f64)) && p->have_fast &&
         !p->exact_gen && !p->generic;
}
// rf_capi.hip rf_can_regenerate_potential
int can_regenerate_potential(const Plan* p, int mode) {
  if (!p || p->unpacked || p->generic || !p->have_fast || p->exact_gen || route(p).replicates()) return 0;
  if (mode == RF_NOISE_NATIVE) return 1;
  if (mode == RF_NOISE_RESIDENT) return (p->has.deviates32() && !p->f64) ? 1 : 0;
  return 0;
}
// rf_capi.hip rf_diag_generation_path
int generation_path(const Plan* p) { return (p->have_fast && !p->exact_gen) ? 1 : 0; }
// rf_capi.hip rf_generate: true = the call goes on
bool generate_ok(const Plan* p, int mode) { return mode != RF_NOISE_RESIDENT || p->has.deviates64(); }
// rf_capi.hip queue_c2r, generic branch (inside `if (!kspace)`): true = the call goes on
bool generic_ok(const Plan* p, const GenParams& gp) { return gp.noise_mode != NOISE_EXTERNAL || p->has.deviates64(); }
// rf_capi_mt.hip rf_noise_mt19937_ex: true = `single` is demoted
bool demotes_single(const Plan* p) { return (p->f64 || p->generic || !p->have_fast || p->exact_gen); }
// rf_capi_mt.hip rf_realise_batch_reference: true = the call goes on
bool batch_reference_ok(const Plan* p) { return route(p).single() && !p->f64 && p->have_fast && !p->exact_gen; }
// rf_capi_mt.hip rf_can_batch_reference (its plan terms): true = "return 0"
bool cannot_batch_reference(const Plan* p) { return !route(p).single() || p->f64 || !p->have_fast || p->exact_gen; }
}  // namespace old

// What the creators, the setters and the replays keep out of the plan's facts, one rule per check that does it
bool facts_reachable(const Plan& p) {
  const bool tiled = rfc::tiled(p.kind);
  // build_fast: `if (... || p->generic) return 0` in front of `have_fast = true`; rf_set_kgrid / rf_set_power, its only callers, refuse an
  // unpacked plan ("this call does not apply to an unpacked c2c plan")
  if (!tiled && p.have_fast) return false;
  // rf_plan_set_flag: the same refusal in front of RF_FLAG_EXACT_GENERATION
  if (p.unpacked && p.exact_gen) return false;
  // every call that leaves deviates (rf_noise_mt19937_ex, rf_mt_share_*, upload_noise's callers) refuses an unpacked plan
  if (p.unpacked && (p.has.d32 || p.has.d64)) return false;
  // float32 pairs come from rf_noise_mt19937_ex, which demotes `single` on float64 and generic plans, and from rf_realise_batch_reference,
  // which refuses them.  (The exact flag set, or the fast records lost to a new power table, AFTER the replay leave the pairs resident:
  // those combinations are reachable, and the first refusal of queue_x is for them.)
  if (p.has.d32 && (p.f64 || !tiled)) return false;
  return true;
}

// ... and what the entry points keep out of a realising call (the x pass of a tiled plan, the generic branch of queue_c2r)
bool call_reachable(const Plan& p, bool kspace, int mode, SourceAsk::Beside beside) {
  if (!facts_reachable(p)) return false;
  // every realising entry point: "this call does not apply to an unpacked c2c plan"
  if (p.unpacked) return false;
  // whoever hands a k-space array over builds a default CallDesc and a NATIVE GenParams (rf_execute_c2r, potential_forward's unfused
  // half, rf_slab_forward_ex(RF_SLAB_FROM_KSPACE)) ...
  if (kspace && (mode != RF_NOISE_NATIVE || beside != SourceAsk::Nothing)) return false;
  // ... and a replicated plan never does: rf_execute_c2r "replicated-generation plans have no distributed k-space buffer",
  // potential_forward "replicated-generation plans keep no k-space potential"; RF_SLAB_FROM_KSPACE needs has.kspace(), which only
  // rf_generate-then-rf_execute_c2r style calls leave and rf_upload_real / the direct set-ups refuse -- kept out here as the first two do
  if (kspace && p.kind == Route::Replicated) return false;
  // upload_noise: "no deviates resident on the device" (RESIDENT); EXTERNAL has just uploaded float64 deviates (deviates64_ready)
  if (mode == RF_NOISE_RESIDENT && !p.has.d32 && !p.has.d64) return false;
  if (mode == RF_NOISE_EXTERNAL && !p.has.d64) return false;
  // pot_target is set by potential_forward alone, behind its own `fused` and its refusal of a replicated plan
  if (beside == SourceAsk::Stored && (!old::fused(&p, mode) || p.kind == Route::Replicated)) return false;
  // emit_potential is set by rf_realise_scaled_potential alone, behind RF_REQUIRE(rf_can_regenerate_potential(p, mode), ...)
  if (beside == SourceAsk::Emitted && !old::can_regenerate_potential(&p, mode)) return false;
  return true;
}

SourceFacts facts(const Plan& p) {
  SourceFacts f;
  f.f64 = p.f64 != 0; f.have_fast = p.have_fast; f.exact_gen = p.exact_gen; f.kind = p.kind;
  f.deviates = p.has.d32 ? SourceFacts::Pairs32 : p.has.d64 ? SourceFacts::Float64 : SourceFacts::None;
  return f;
}
bool same_text(const char* a, const char* b) { return a && b && std::strcmp(a, b) == 0; }

}  // namespace

int main() {
  int n_reachable = 0, n_excluded = 0, n_beside_refused = 0, n_kept = 0;
  const Route::Kind kinds[] = {Route::C2C, Route::Generic, Route::Single, Route::Replicated, Route::Exchange};
  const char* const kind_names[] = {"c2c", "generic", "single", "replicated", "exchange"};
  const SourceAsk::Beside besides[] = {SourceAsk::Nothing, SourceAsk::Stored, SourceAsk::Emitted};
  const int dummy = 0;
  for (int bits = 0; bits < 8; ++bits)
    for (int ki = 0; ki < 5; ++ki)
      for (int dev = 0; dev < 3; ++dev)
        for (int ks = 0; ks < 2; ++ks)
          for (int mode = 0; mode < 3; ++mode)
            for (SourceAsk::Beside beside : besides) {
              Plan p{bits & 1, (bits & 2) != 0, (bits & 4) != 0, kinds[ki] == Route::Generic, kinds[ki] == Route::C2C, kinds[ki], Has{dev == 1, dev == 2}};
              const bool kspace = ks != 0;
              std::snprintf(g_where, sizeof(g_where), "f64=%d have_fast=%d exact_gen=%d kind=%s deviates=%s kspace=%d mode=%d beside=%d", p.f64,
                            p.have_fast, p.exact_gen, kind_names[ki], dev == 1 ? "pairs32" : dev == 2 ? "float64" : "none", ks, mode, (int)beside);
              const SourceFacts f = facts(p);
              const Source s = rfc::source_of(f, SourceAsk::x_pass(kspace, mode, beside));
              // total: a kind or a refusal with one of the texts; the accessors follow the kind
              CHECK(s.kind >= Source::Refused && s.kind <= Source::FastDeviates64);
              CHECK(s.refused() == (s.refusal != nullptr));
              if (s.refused())
                CHECK(same_text(s.refusal, T_PAIRS_ONLY) || same_text(s.refusal, T_REPLICATED) || same_text(s.refusal, T_GENERIC) || same_text(s.refusal, T_BESIDE));
              CHECK((int)s.fast() + (int)(s.kind == Source::ExactPhilox) + (int)(s.kind == Source::ExactDeviates64) + (int)(s.kind == Source::GivenKspace) + (int)s.refused() == 1);
              CHECK(!s.reads_pairs32() || s.fast());
              CHECK(s.stores_potential() == (!s.refused() && beside == SourceAsk::Stored) && s.emits_potential() == (!s.refused() && beside == SourceAsk::Emitted));
              if (same_text(s.refusal, T_BESIDE)) ++n_beside_refused;

              // ---- the predicates, which a caller may ask at any time: on every plan the creators and setters allow ----
              if (facts_reachable(p) && !kspace) {
                if (mode == RF_NOISE_NATIVE && beside == SourceAsk::Nothing) {      // (they take no mode and no ask: once per plan)
                  CHECK(old::generation_path(&p) == (int)s.fast());                 // rf_diag_generation_path asks a NATIVE x pass
                  CHECK(old::demotes_single(&p) == !rfc::resident_reads_pairs32(f));
                  CHECK(old::batch_reference_ok(&p) == (route(&p).single() && rfc::resident_reads_pairs32(f)));
                  CHECK(old::cannot_batch_reference(&p) == !(route(&p).single() && rfc::resident_reads_pairs32(f)));
                }
                if (beside == SourceAsk::Emitted) CHECK(old::can_regenerate_potential(&p, mode) == (int)s.emits_potential());
                // potential_forward asks BEFORE upload_noise: every deviate state under every mode; behind "does not apply to an unpacked
                // c2c plan" (rf_realise_potential, rf_slab_forward_ex) and its own refusal of a replicated plan
                if (beside == SourceAsk::Stored && !p.unpacked && p.kind != Route::Replicated) CHECK(old::fused(&p, mode) == s.stores_potential());
                // rf_generate: behind the unpacked refusal and upload_noise
                if (beside == SourceAsk::Nothing && !p.unpacked && !(mode == RF_NOISE_RESIDENT && dev == 0) && !(mode == RF_NOISE_EXTERNAL && dev != 2)) {
                  const Source sg = rfc::source_of(f, SourceAsk::fill_k(mode));
                  CHECK(old::generate_ok(&p, mode) == !sg.refused());
                  if (sg.refused()) CHECK(same_text(sg.refusal, T_GENERATE));
                  else CHECK(sg.kind == (mode == RF_NOISE_NATIVE ? Source::ExactPhilox : Source::ExactDeviates64));      // launch_gen_kspace: the exact chain
                }
              }

              // ---- the realising call ----
              if (!call_reachable(p, kspace, mode, beside)) { ++n_excluded; continue; }
              ++n_reachable;
              const GenParams gp = make_gen(mode);
              CallDesc cd;
              cd.resident_fast = (mode == RF_NOISE_RESIDENT);
              cd.pot_target = beside == SourceAsk::Stored ? &dummy : nullptr;
              cd.emit_potential = beside == SourceAsk::Emitted;
              CHECK(!same_text(s.refusal, T_BESIDE));
              if (p.generic) {                      // queue_c2r's generic branch: launch_gen_kspace / the generating generic x pass, the exact chain
                const bool ok = kspace || old::generic_ok(&p, gp);
                CHECK(ok == !s.refused());
                if (!ok) CHECK(same_text(s.refusal, T_GENERIC));
                else CHECK(s.kind == (kspace ? Source::GivenKspace : mode == RF_NOISE_NATIVE ? Source::ExactPhilox : Source::ExactDeviates64));
                continue;
              }
              const old::X x = old::queue_x(&p, cd, gp, kspace ? &dummy : nullptr);
              CHECK((x.refusal != nullptr) == s.refused());
              if (x.refusal) { CHECK(same_text(x.refusal, s.refusal)); continue; }
              CHECK(x.fast == s.fast());                                           // launch_col_fastgen / launch_col_gen
              CHECK(x.noise32 == s.reads_pairs32());                               // fgp.noise32, fgp.rowtab, fgp.seg_cap
              CHECK(x.noise == (s.kind == Source::FastDeviates64));                // fgp.noise
              if (!x.fast)                                                         // what launch_col_gen loads: K, or gp.noise under gp.noise_mode, or Philox
                CHECK(s.kind == (kspace ? Source::GivenKspace : gp.noise_mode == NOISE_EXTERNAL ? Source::ExactDeviates64 : Source::ExactPhilox));
              else if (!x.noise32 && !x.noise) CHECK(s.kind == Source::FastPhilox);
              // the fast kernel got pot_target and emit_potential whatever it read; both asks are now granted by name
              CHECK(s.stores_potential() == (cd.pot_target != nullptr) && s.emits_potential() == cd.emit_potential);
            }
  // The one place where two old spellings disagree on a reachable combination, by name: "replicated plan, float32 replay".
  // rf_noise_mt19937_ex does not demote `single` there (its test has no term for replication), yet no x pass of a replicated plan reads
  // the pairs: rf_realise(RF_NOISE_RESIDENT) is refused with the float32-copies text.  Before = after: the replay still leaves float32
  // pairs, and the realisation is still refused at the same point with the same text (demoting the replay would have let
  // rf_download_noise and rf_generate(RF_NOISE_RESIDENT) succeed where they were refused).
  for (int fast_on = 0; fast_on < 2; ++fast_on) {
    Plan p{0, true, fast_on == 0, false, false, Route::Replicated, Has{true, false}};
    std::snprintf(g_where, sizeof(g_where), "replicated plan, float32 replay, exact_gen=%d", (int)p.exact_gen);
    const Source s = rfc::source_of(facts(p), SourceAsk::x_pass(false, RF_NOISE_RESIDENT));
    CallDesc cd;
    cd.resident_fast = true;
    CHECK(!old::demotes_single(&p) == rfc::resident_reads_pairs32(facts(p)));
    CHECK(same_text(old::queue_x(&p, cd, make_gen(RF_NOISE_RESIDENT), nullptr).refusal, T_PAIRS_ONLY) && same_text(s.refusal, T_PAIRS_ONLY));
    ++n_kept;
  }
  CHECK(n_beside_refused > 0);
  std::printf("combinations: %d reachable, %d excluded (an unservable potential ask is refused on %d of the excluded, on none of the reachable)\n",
              n_reachable, n_excluded, n_beside_refused);
  std::printf("old spellings that disagree on a reachable plan: replicated plan + float32 replay (%d variants), outcome kept\n", n_kept);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  if (g_failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
