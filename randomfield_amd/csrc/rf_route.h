// rf_route.h -- which pipeline a plan runs: the one decision behind every "is this a slab plan / does it exchange / does it replicate"
// of the C-API layer.  A plan is exactly one of five kinds; an exchanging one moves its data either by grouped send / receive or by the
// storing ("direct") y pass, each whole or in sub-slabs.  The entry points ask route(p) (rf_plan.h), which fills the facts from the
// plan and calls route_of: computed per question, never cached, so no setter has a copy to refresh.  Plain C++, no HIP
// (tests/route_test.cpp walks every combination of the facts on the CPU).  DESIGN.md section 3.21 has the table in words.
//
// Conditions that ask ANOTHER question stay as they are and do not come here: "one rank" (`p->nranks == 1` of the gradient, Hessian,
// 2LPT, particle and P(k) calls and of the graph-captured batch), "more than one rank" (`p->nranks > 1` of rf_slab_*, of the
// communicator and of rf_execute_r2c's branch), the per-entry-point refusals of c2c / generic plans by their own texts, and the
// `p->direct` of RF_FLAG_EXCHANGE_CHUNKS, which keeps the destination table of a direct mode that is set up in step with the chunks
// whether or not the plan exchanges at the moment.
#pragma once

namespace rfc {

// the plan's raw facts, as its creators and setters leave them
struct RouteFacts {
  bool unpacked = false;      // rf_plan_create_c2c
  bool generic = false;       // an axis that is no power of two (either creator)
  int nranks = 1;
  bool force_slab = false;    // RF_FLAG_FORCE_SLAB_PATH
  bool replicate = false;     // RF_FLAG_REPLICATED_GENERATION
  bool direct = false;        // the storing y pass is set up (rf_comm_enable_direct, rf_slab_link_direct, rf_slab_direct_import, rf_slab_set_direct_standin)
  int xchunks = 1;            // RF_FLAG_EXCHANGE_CHUNKS
};

struct Route {
  enum Kind { C2C, Generic, Single, Replicated, Exchange };
  Kind kind = Single;
  bool direct = false;        // Exchange only: the y pass stores into the peers' receive buffers (else grouped send / receive)
  int chunks = 1;             // Exchange only: sub-slabs of the kz slab, each exchanged on its own (1: the whole slab at once)

  bool exchanges() const { return kind == Exchange; }      // an exchange between the y and z passes: multi-rank, or one rank forced onto the slab path
  bool single() const { return kind == Single; }           // the single-GPU tiled pipeline (queue_xyz: slabs of x planes, merged launches, graphs, host sink)
  bool replicates() const { return kind == Replicated; }   // multi-rank without an exchange: every rank generates all of k space
};

// Total: every combination of the facts has a kind.  The order is the precedence, and it only matters on combinations the setters keep
// out -- on those the spellings this function replaced disagreed with one another (tests/route_test.cpp lists them):
//   unpacked            => one rank, no flag of the slab path: rf_plan_create_c2c sets nranks = 1, and rf_plan_set_flag refuses an
//                          unpacked plan ("this call does not apply to an unpacked c2c plan") as do rf_comm_enable_direct and the rf_slab_* set-ups
//   generic             => one rank (rf_plan_create: `generic = nranks == 1 && ...`); never forced onto the slab path
//                          ("RF_FLAG_FORCE_SLAB_PATH needs power-of-two axes"), never chunked ("RF_FLAG_EXCHANGE_CHUNKS is for packed
//                          plans on the tiled kernels"), never direct (direct_shape_ok, rf_capi_slab.hip)
//   replicate           => more than one rank ("RF_FLAG_REPLICATED_GENERATION is for multi-rank plans")
//   force_slab          => one rank ("RF_FLAG_FORCE_SLAB_PATH is for single-rank plans")
// `direct` and `xchunks` may be set on a plan that does not exchange (the flag of the forced slab path cleared again, replication
// switched on afterwards): they then mean nothing, and the route says so.
inline Route route_of(const RouteFacts& f) {
  Route r;
  if (f.unpacked) r.kind = Route::C2C;
  else if (f.generic) r.kind = Route::Generic;
  else if (f.nranks == 1 && !f.force_slab) r.kind = Route::Single;
  else if (f.replicate && f.nranks > 1) r.kind = Route::Replicated;
  else r.kind = Route::Exchange;
  if (r.kind == Route::Exchange) {
    r.direct = f.direct;
    r.chunks = f.xchunks > 1 ? f.xchunks : 1;
  }
  return r;
}

}  // namespace rfc
