// route_test.cpp -- which pipeline a plan runs (randomfield_amd/csrc/rf_route.h) against the spellings it replaced.  The functions of
// namespace old below are LITERAL COPIES of the expressions the C-API layer worked the answer out with before the change, over a
// struct that has the plan's seven members of that name.  Every combination of the seven facts is walked: nranks in {1, 2, 4}, xchunks
// in {1, 2, 4} and the five bools.  On every combination the creators and setters allow, each old expression must equal the
// route's answer; on the excluded ones -- where the old spellings disagree with one another, which is why they needed the setters --
// the route must still name a kind.  Stand-alone: compiled with -fsanitize=address,undefined and run by tests/test_route.py; exit
// status 0 = every check held.
#include <cstdio>

#include "../randomfield_amd/csrc/rf_route.h"

namespace {

using rfc::Route;
using rfc::RouteFacts;

int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) { std::printf("FAILED %s:%d: %s   [%s]\n", __FILE__, __LINE__, #cond, g_where); ++g_failed; } \
  } while (0)
char g_where[160];

// the seven plan members the old expressions read
struct Plan {
  bool unpacked, generic;
  int nranks;
  bool force_slab, replicate, direct;
  int xchunks;
  bool xposed = true;          // (RF_FLAG_TRANSPOSED_INTERMEDIATE set, so that the first line of xpose_ok decides)
  int yz_slab = -1;            // (not 0, so that the first line of yz_slab_planes decides)
};

namespace old {
// rf_capi.hip slab_chunks
int slab_chunks(const Plan* p) {
  return (p->xchunks > 1 && (p->nranks > 1 || p->force_slab) && !p->replicate && !p->generic && !p->unpacked) ? p->xchunks : 1;
}
// rf_capi.hip direct_active
bool direct_active(const Plan* p) {
  return p->direct && (p->nranks > 1 || p->force_slab) && !p->replicate && !p->generic && !p->unpacked;
}
// rf_capi.hip xpose_ok, first line: true = "return false" taken
bool xpose_refused(const Plan* p) {
  if (!p->xposed || p->generic || p->unpacked || p->nranks > 1 || p->force_slab) return true;
  return false;
}
// rf_capi.hip yz_slab_planes, first line: true = "return 0" taken
bool yz_whole_grid(const Plan* p) {
  if (p->nranks > 1 || p->force_slab || p->generic || p->unpacked || p->yz_slab == 0) return true;
  return false;
}
// rf_capi.hip queue_c2r: the if-ladder, as "which branch"
enum Branch { GENERIC, SINGLE, DIRECT, CHUNKED, REPLICATED, WHOLE, UNREACHABLE };
Branch queue_c2r(const Plan* p) {
  if (p->generic) return GENERIC;
  if (p->nranks == 1 && !p->force_slab) return SINGLE;
  if (direct_active(p)) return DIRECT;
  if (slab_chunks(p) > 1) return CHUNKED;
  if (p->replicate && p->nranks > 1) return REPLICATED;
  if (p->nranks > 1 || p->force_slab) return WHOLE;
  return UNREACHABLE;
}
// rf_capi.hip rf_realise_batch: slab_batch / the generic loop / the captured graph; inside slab_batch: back to back / direct / rccl
enum Batch { B_REPLICATED, B_DIRECT, B_RCCL, B_GENERIC, B_GRAPH };
Batch realise_batch(const Plan* p) {
  if (p->nranks > 1 || p->force_slab) {
    if (p->replicate && p->nranks > 1) return B_REPLICATED;
    if (direct_active(p)) return B_DIRECT;
    return B_RCCL;
  }
  if (p->generic) return B_GENERIC;
  return B_GRAPH;
}
// rf_capi.hip rf_realise_batch_prepare: true = "return 0" (nothing to capture)
bool batch_not_captured(const Plan* p) { return p->nranks > 1 || p->force_slab || p->generic; }
// rf_capi.hip rf_realise_scaled_potential: fuse_z without its factor_z and xpose_ok terms
bool fuse_z(const Plan* p) { return p->nranks == 1 && !p->force_slab; }
// the conditions of the refusals (true = the call goes on)
bool lognormal_ok(const Plan* p) { return p->nranks == 1 && !p->force_slab && !p->generic; }                          // rf_realise_lognormal
bool host_sink_ok(const Plan* p) { return !p->unpacked && !p->generic && p->nranks == 1 && !p->force_slab; }          // rf_set_host_sink
bool batch_reference_ok(const Plan* p) { return p->nranks == 1 && !p->force_slab && !p->generic; }                    // rf_realise_batch_reference (its route terms)
bool cannot_batch_reference(const Plan* p) { return p->unpacked || p->nranks != 1 || p->force_slab || p->generic; }   // rf_can_batch_reference (its route terms)
// the two spellings of "replicates": queue_x, queue_xy, slab_batch, queue_c2r, rf_execute_c2r, rf_can_regenerate_potential,
// potential_forward, rf_upload_real / the direct set-ups of rf_capi_slab.hip, rf_mt_share_begin
bool replicates_guarded(const Plan* p) { return p->replicate && p->nranks > 1; }
bool replicates_bare(const Plan* p) { return p->replicate; }
// rf_execute_r2c, inside its `p->nranks > 1` branch
bool r2c_multi_ok(const Plan* p) { return !p->generic && !p->replicate; }
}  // namespace old

// What the creators and the setters keep out, one rule per check that does it (the texts are the refusals' own).  A combination is
// reachable when no rule excludes it.  `direct` and `xchunks` outlive what they were set for -- RF_FLAG_FORCE_SLAB_PATH cleared again,
// RF_FLAG_REPLICATED_GENERATION set afterwards, RF_FLAG_EXCHANGE_CHUNKS on a single-rank plan -- so those combinations ARE reachable,
// and the old spellings had to agree on them too.
bool reachable(const Plan& p) {
  // rf_plan_create_c2c: `p->nranks = 1`
  if (p.unpacked && p.nranks != 1) return false;
  // rf_plan_set_flag: "this call does not apply to an unpacked c2c plan" in front of every flag of the slab path
  if (p.unpacked && (p.force_slab || p.replicate || p.xchunks != 1)) return false;
  // rf_comm_enable_direct, rf_slab_direct_import, rf_slab_set_direct_standin: the same refusal; rf_slab_link_direct: direct_shape_ok
  if (p.unpacked && p.direct) return false;
  // rf_plan_create: `generic = nranks == 1 && generic_dims(...)`
  if (p.generic && p.nranks != 1) return false;
  // rf_plan_set_flag: "RF_FLAG_FORCE_SLAB_PATH needs power-of-two axes"
  if (p.generic && p.force_slab) return false;
  // rf_plan_set_flag: "RF_FLAG_EXCHANGE_CHUNKS is for packed plans on the tiled kernels"
  if (p.generic && p.xchunks != 1) return false;
  // every set-up of the direct mode asks direct_shape_ok (rf_capi_slab.hip), which refuses a generic plan
  if (p.generic && p.direct) return false;
  // rf_plan_set_flag: "RF_FLAG_REPLICATED_GENERATION is for multi-rank plans"
  if (p.replicate && p.nranks == 1) return false;
  // rf_plan_set_flag: "RF_FLAG_FORCE_SLAB_PATH is for single-rank plans"
  if (p.force_slab && p.nranks != 1) return false;
  return true;
}

Route route(const Plan& p) {
  RouteFacts f;
  f.unpacked = p.unpacked; f.generic = p.generic; f.nranks = p.nranks; f.force_slab = p.force_slab;
  f.replicate = p.replicate; f.direct = p.direct; f.xchunks = p.xchunks;
  return rfc::route_of(f);
}

// the branch of the new queue_c2r: a switch over the kind, the exchanging forms told apart by direct and chunks
old::Branch new_branch(const Route& r) {
  switch (r.kind) {
    case Route::C2C: return old::UNREACHABLE;          // (refused by every caller before queue_c2r)
    case Route::Generic: return old::GENERIC;
    case Route::Single: return old::SINGLE;
    case Route::Replicated: return old::REPLICATED;
    case Route::Exchange: return r.direct ? old::DIRECT : r.chunks > 1 ? old::CHUNKED : old::WHOLE;
  }
  return old::UNREACHABLE;
}
old::Batch new_batch(const Route& r) {
  if (r.replicates()) return old::B_REPLICATED;
  if (r.exchanges()) return r.direct ? old::B_DIRECT : old::B_RCCL;
  return r.kind == Route::Generic ? old::B_GENERIC : old::B_GRAPH;
}

}  // namespace

int main() {
  int n_reachable = 0, n_excluded = 0, n_old_disagree = 0;
  const int ranks[] = {1, 2, 4}, chunks[] = {1, 2, 4};
  for (int bits = 0; bits < 32; ++bits)
    for (int nr : ranks)
      for (int xc : chunks) {
        Plan p{(bits & 1) != 0, (bits & 2) != 0, nr, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, xc};
        std::snprintf(g_where, sizeof(g_where), "unpacked=%d generic=%d nranks=%d force_slab=%d replicate=%d direct=%d xchunks=%d", p.unpacked,
                      p.generic, p.nranks, p.force_slab, p.replicate, p.direct, p.xchunks);
        const Route r = route(p);
        // total: a kind on every combination, exactly one reader or one of the two kinds without one, and the two details on Exchange only
        CHECK(r.kind == Route::C2C || r.kind == Route::Generic || r.kind == Route::Single || r.kind == Route::Replicated || r.kind == Route::Exchange);
        CHECK((int)r.exchanges() + (int)r.single() + (int)r.replicates() + (int)(r.kind == Route::C2C) + (int)(r.kind == Route::Generic) == 1);
        CHECK(r.chunks >= 1 && (r.exchanges() || (!r.direct && r.chunks == 1)));
        if (!reachable(p)) {
          ++n_excluded;
          // the old spellings need the setters: somewhere in the excluded set each pair below falls apart
          if (old::replicates_guarded(&p) != old::replicates_bare(&p) || old::queue_c2r(&p) == old::UNREACHABLE ||
              old::xpose_refused(&p) != old::yz_whole_grid(&p) || old::host_sink_ok(&p) != old::lognormal_ok(&p))
            ++n_old_disagree;
          continue;
        }
        ++n_reachable;
        CHECK(old::slab_chunks(&p) == r.chunks);
        CHECK(old::direct_active(&p) == r.direct);
        CHECK(old::xpose_refused(&p) == !r.single());
        CHECK(old::yz_whole_grid(&p) == !r.single());
        CHECK(old::host_sink_ok(&p) == r.single());
        CHECK(old::cannot_batch_reference(&p) == !r.single());
        CHECK(old::replicates_guarded(&p) == r.replicates());
        CHECK(old::replicates_bare(&p) == r.replicates());
        if (p.nranks > 1) CHECK(old::r2c_multi_ok(&p) == r.exchanges());
        if (p.unpacked) {               // every entry point below refuses an unpacked plan before it asks
          CHECK(r.kind == Route::C2C);
          continue;
        }
        CHECK(old::queue_c2r(&p) != old::UNREACHABLE);
        CHECK(old::queue_c2r(&p) == new_branch(r));
        CHECK(old::realise_batch(&p) == new_batch(r));
        CHECK(old::batch_not_captured(&p) == !r.single());
        CHECK(old::lognormal_ok(&p) == r.single());
        CHECK(old::batch_reference_ok(&p) == r.single());
        if (!p.generic) CHECK(old::fuse_z(&p) == r.single());      // (rf_can_regenerate_potential has refused a generic plan before)
      }
  CHECK(n_old_disagree > 0);
  std::printf("combinations: %d reachable, %d excluded (the old spellings disagree with one another on %d of the excluded)\n", n_reachable,
              n_excluded, n_old_disagree);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  if (g_failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
