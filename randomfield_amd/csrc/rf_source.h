// rf_source.h -- which generator fills an x pass, where its deviates come from, and whether it can also store or emit the potential: the
// one decision behind every "fast or exact kernel / float32 pairs or float64 deviates / can this call have the potential too" of the
// C-API layer.  The entry points ask source(p, ask) (rf_plan.h), which fills the facts from the plan as they are at the moment of the
// call and calls source_of: computed per call, never cached, so no setter and no replay has a copy to refresh.  Plain C++, no HIP
// (tests/source_test.cpp walks every combination of facts and asks on the CPU).  DESIGN.md section 3.22 has the table in words.
//
// Conditions that ask ANOTHER question stay as they are and do not come here: rf_mt_share_begin's `single && p->f64` (the precision of
// the distributed replay's TRANSPORT; what it leaves is always float64 deviates), upload_noise's checks (whether deviates ARE resident /
// a host array was given -- this decision starts from what is resident), the refusals of an invalid noise mode with their two texts
// ("invalid noise mode" / "unknown noise mode"), build_fast (whether the fast records CAN be built: it makes the fact `have_fast`), and
// everything about `fused_generic`, which says WHERE a generic plan runs its generation (inside the x pass or into K first), not which
// generator runs: a generic plan always runs the exact chain.  The segment-length test of the float32 replay
// (`g.cap >= 4 (nzc + 1)`, rf_capi_mt.hip) asks whether the replay can MAKE float32 pairs on this grid, not whether anything reads them.
#pragma once
#include "rf_route.h"

namespace rfc {

// what the plan contributes
struct SourceFacts {
  bool f64 = false;                    // complex128 plan
  bool have_fast = false;              // the fast generation pass's records exist (build_fast)
  bool exact_gen = false;              // RF_FLAG_EXACT_GENERATION
  Route::Kind kind = Route::Single;    // the pipeline the plan runs (rf_route.h)
  enum Deviates { None, Pairs32, Float64 };
  Deviates deviates = None;            // what is resident on the device (rf_contents.h: deviates32() / deviates64())
};

// what the call contributes
struct SourceAsk {
  bool kspace = false;                 // the x pass transforms a given k-space array: nothing is generated
  bool fills_k = false;                // rf_generate: the exact chain writes the API-layout k-space array, whatever an x pass of the plan would run
  enum Mode { Native = 0, External = 1, Resident = 2 };      // the noise mode as the API names and numbers it (RF_NOISE_*; rf_plan.h checks the numbers)
  Mode mode = Native;
  enum Beside { Nothing, Stored, Emitted };      // beside delta(k): delta(k) / k^2 stored (pot_target), or the scaled potential in its place (emit_potential)
  Beside beside = Nothing;

  // (the entry points have refused any other number by their own texts, "invalid noise mode" / "unknown noise mode")
  static Mode mode_of(int api_mode) { return api_mode == Resident ? Resident : api_mode == External ? External : Native; }
  // the ask of an x pass (kspace: it transforms that array), and of rf_generate
  static SourceAsk x_pass(bool kspace, int api_mode, Beside beside = Nothing) {
    SourceAsk a;
    a.kspace = kspace; a.mode = mode_of(api_mode); a.beside = beside;
    return a;
  }
  static SourceAsk fill_k(int api_mode) {
    SourceAsk a;
    a.fills_k = true; a.mode = mode_of(api_mode);
    return a;
  }
};

struct Source {
  enum Kind { Refused, GivenKspace, ExactPhilox, ExactDeviates64, FastPhilox, FastPairs32, FastDeviates64 };
  Kind kind = Refused;
  const char* refusal = nullptr;       // Refused only: the text the entry point fails with
  SourceAsk::Beside beside = SourceAsk::Nothing;      // the ask, granted (a source that cannot serve it is Refused)

  bool refused() const { return kind == Refused; }
  bool fast() const { return kind == FastPhilox || kind == FastPairs32 || kind == FastDeviates64; }      // the fast kernel (else the exact one)
  bool reads_pairs32() const { return kind == FastPairs32; }                       // wires noise32 / rowtab / seg_cap
  bool stores_potential() const { return !refused() && beside == SourceAsk::Stored; }
  bool emits_potential() const { return !refused() && beside == SourceAsk::Emitted; }
};

inline bool tiled(Route::Kind k) { return k == Route::Single || k == Route::Replicated || k == Route::Exchange; }

// "The generator a RESIDENT realisation of this plan runs reads float32 pairs": what rf_noise_mt19937_ex asks before it honours
// `single` (else the replay is demoted to float64 deviates), and the plan half of rf_realise_batch_reference / rf_can_batch_reference.
// About the GENERATOR, not the route: a replicated plan refuses every RESIDENT x pass (below), and its replay is still not demoted --
// as before, so that what reads float64 deviates only (rf_download_noise, rf_generate) stays refused after a float32 replay there.
inline bool resident_reads_pairs32(const SourceFacts& f) { return tiled(f.kind) && !f.f64 && f.have_fast && !f.exact_gen; }

// Total: every combination of facts and ask gets a kind or a refusal.  In words:
//   a given k-space array        is transformed as it is;
//   NATIVE                       the fast kernel on Philox where the plan has it (tiled kernels, records built, exact flag off), else the
//                                exact kernel on Philox;
//   RESIDENT                     on a plan whose fast kernel reads float32 pairs (resident_reads_pairs32) and that does not replicate: the
//                                fast kernel on the pairs, or on float64 deviates when those are what is resident;
//   RESIDENT otherwise, EXTERNAL the exact kernel on float64 deviates -- refused when there are none;
//   rf_generate (fills_k)        always the exact chain;
//   a replicated plan            runs the fast kernel on Philox and nothing else (rf_generate aside, which runs no x pass);
//   the potential, beside        from the fast kernel on Philox or on float32 pairs only (the float64 deviates' form of the fast kernel
//                                and the exact kernel have no second store stream and no scaled form), and never on a replicated plan.
inline Source source_of(const SourceFacts& f, const SourceAsk& a) {
  auto refuse = [](const char* why) { Source s; s.refusal = why; return s; };
  const bool rep = f.kind == Route::Replicated;
  const bool x_pass = !a.fills_k;
  Source s;
  s.beside = a.beside;
  if (a.kspace) s.kind = Source::GivenKspace;
  else if (a.mode == SourceAsk::Native)
    s.kind = (x_pass && tiled(f.kind) && f.have_fast && !f.exact_gen) ? Source::FastPhilox : Source::ExactPhilox;
  else if (a.mode == SourceAsk::Resident && x_pass && resident_reads_pairs32(f) && !rep && f.deviates != SourceFacts::None)
    s.kind = f.deviates == SourceFacts::Pairs32 ? Source::FastPairs32 : Source::FastDeviates64;
  else if (f.deviates == SourceFacts::Float64) s.kind = Source::ExactDeviates64;
  else if (a.fills_k) return refuse("rf_generate needs float64 deviates: only float32 copies are resident");
  else if (!tiled(f.kind)) return refuse("no float64 deviates resident on the device");
  else
    return refuse("only float32 copies of the deviates are resident: this path (exact chain / float64 plan) needs rf_noise_mt19937's float64 ones");
  if (rep && x_pass && s.kind != Source::FastPhilox) return refuse("replicated generation needs the native generator (fast path)");
  // (no entry point FAILS with this text: potential_forward and rf_can_regenerate_potential ask here first and read it as "no")
  if (a.beside != SourceAsk::Nothing && (rep || (s.kind != Source::FastPhilox && s.kind != Source::FastPairs32)))
    return refuse("this generation source cannot store or emit the potential");
  return s;
}

}  // namespace rfc
