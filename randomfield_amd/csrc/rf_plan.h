// rf_plan.h -- the plan object behind the C-ABI and the helpers its translation units share (rf_capi.hip: plans, inputs,
// realisations, transforms, host <-> device; rf_capi_mt.hip: the MT19937 replay and its sharing between ranks; rf_capi_slab.hip: the
// communicator and the slab pipeline in separate steps).  What the plan's buffers HOLD belongs to none of the three: it is the member
// `has` (rf_contents.h), asked and changed through its predicates and transitions only; WHICH PIPELINE the plan runs is route(p) (rf_route.h) and
// WHICH GENERATOR fills an x pass source(p, ask) (rf_source.h), worked out from the plan's facts per question.  Internal: nothing here crosses the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/randomfield_hip.h"
#include "../../include/randomfield_hip_diag.h"
#include "rf_contents.h"
#include "rf_host.h"
#include "rf_launch.h"
#include "rf_owned.h"
#include "rf_replay.h"
#include "rf_route.h"
#include "rf_select.h"
#include "rf_source.h"
#include "rf_timing.h"

namespace rfc {
using namespace rf;


extern thread_local std::string g_err;      // last error message of the calling thread (rf_last_error)
int fail(int code, const std::string& msg);

#define RF_HIP(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(2, std::string(#expr) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                         std::to_string(__LINE__) + ")");                                         \
  } while (0)

#define RF_REQUIRE(cond, msg) \
  do {                        \
    if (!(cond)) return fail(1, msg); \
  } while (0)
// ... where a function of the HIP-free headers hands the refusal's text back (nullptr: none)
#define RF_REFUSE(why)                              \
  do {                                              \
    if (const char* w_ = (why)) return fail(1, w_); \
  } while (0)

// RCCL entry points, resolved lazily with dlopen so that single-GPU use never depends on librccl
// being loadable (types and enums come from <rccl/rccl.h>, no link-time dependency).
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
extern Rccl g_rccl;
int load_rccl();

#define RF_NCCL(expr)                                                                                   \
  do {                                                                                                  \
    ncclResult_t r_ = (expr);                                                                           \
    if (r_ != ncclSuccess)                                                                              \
      return fail(5, std::string(#expr) + " failed: " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?")); \
  } while (0)

// the HIP runtime behind the owning handles of rf_owned.h: device memory, events and streams; pinned host memory
struct HipApi {
  using Error = hipError_t;
  using Event = hipEvent_t;
  using Stream = hipStream_t;
  static constexpr Error ok = hipSuccess;
  static constexpr bool device = true;
  static Error alloc(void** q, size_t n) { return hipMalloc(q, n); }
  static Error free(void* q) { return hipFree(q); }
  static Error event_create(Event* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
  static Error event_destroy(Event e) { return hipEventDestroy(e); }
  static constexpr Error not_ready = hipErrorNotReady;      // (rf_timing.h: a read-out before a call has finished)
  static Error event_record(Event e, Stream s) { return hipEventRecord(e, s); }
  static Error event_sync(Event e) { return hipEventSynchronize(e); }
  static Error event_elapsed(float* ms, Event from, Event to) { return hipEventElapsedTime(ms, from, to); }
  static Error stream_create(Stream* s, unsigned flags) { return hipStreamCreateWithFlags(s, flags); }
  static Error stream_destroy(Stream s) { return hipStreamDestroy(s); }
};
struct HipPinned : HipApi {
  static constexpr bool device = false;
  static Error alloc(void** q, size_t n) { return hipHostMalloc(q, n, hipHostMallocDefault); }
  static Error free(void* q) { return hipHostFree(q); }
};
template <class T = void> using DevBuf = rfo::Buffer<HipApi, T>;
using Events = rfo::EventList<HipApi>;
using OwnedStream = rfo::Stream<HipApi>;
using Timeline = rft::Timeline<HipApi>;
using rft::Part;

// a mark of the call's timeline where a schedule has one (tl == nullptr: the call is not timed; rf_timing.h)
inline hipError_t mark(Timeline* tl, Part part, hipStream_t s, hipEvent_t* out = nullptr, bool merged = false) {
  return tl ? tl->mark(part, s, out, merged) : hipSuccess;
}
// stream `to` goes on once stream `from` has come this far
inline hipError_t hop(hipEvent_t e, hipStream_t from, hipStream_t to) {
  if (hipError_t r = hipEventRecord(e, from); r != hipSuccess) return r;
  return hipStreamWaitEvent(to, e, 0);
}

// The MT19937 replay of a plan (rf_capi_mt.hip; the host arithmetic is rf_replay.h): the uploaded jump table, the device buffers of one
// replay, the shared replay of a kz-slab job, the block of rf_realise_batch_reference.
struct MtReplay {
  JumpTable table;                     // what rf_mt_set_jump keeps on the host
  DevBuf<uint32_t> pos;                // the table's device rows (rf_replay.h widen_jump_table) ...
  DevBuf<int> npos_dev;                // ... and their four padded counts per polynomial
  bool table_uploaded() const { return table.uploaded(pos.get()); }
  DevBuf<uint32_t> states;
  DevBuf<unsigned long long> counts, offsets;
  DevBuf<> scratch;                    // one-pass replay: every segment's accepted pairs, densely from slot seg * (attempts per segment)
  // float32 deviates (rf_noise_mt19937_ex(single = 1)) stay where the one-pass replay writes them: scratch, every segment's accepted
  // pairs from slot seg * seg_cap, located through offsets (FastGenParams::seg_*): has.deviates32().  Only one of the two forms
  // (float64 in cell order in `noise` / float32 in segment order) is valid at a time.
  unsigned long long seg_cap = 0;
  int nseg = 0;
  DevBuf<> rowtab;                     // float32 form: where each row (ix, iy) of the stream starts in the runs (rf_core.h RowLoc, 8 B x nx ny)
  DevBuf<int> flags;                   // device word: bit 0 = a row spans more than two segments (mt_rowtab_kernel)
  // distributed replay (rf_mt_share_*): this rank replays segments [sh_first, sh_first + sh_nloc) of the one stream
  DevBuf<> send, recv;                 // pairs packed by destination rank / stream of this rank as received (float32 mode)
  DevBuf<long long> sbase;             // device, [nranks]: see mt_share_pack_kernel
  DevBuf<unsigned long long> first;    // device: first stream cell of every local segment
  ShareStep step;                      // which of the share calls has run, and the mode of the transport (float32 pairs / float64)
  int sh_first = 0, sh_nloc = 0;       // rf_mt_share_begin: this rank's first segment and the number of its segments
  ShareSplit split;                    // rf_mt_share_pack: what this rank sends to and receives from every peer
  // rf_realise_batch_reference: [start states n x 624][accepted totals n][flags n], kept between calls (allocating and freeing them
  // cost a device synchronisation per call: one-seed batches are the Generator's call); its events: replay finished / generation pass
  // has read the runs
  DevBuf<> br_tmp;
  int br_cap = 0;
  Events bev;
};

}  // namespace rfc

// Everything the plan allocates is a member of an owning type (rf_owned.h): rf_plan_destroy drains the streams and deletes the plan.
// Members die in reverse order of declaration, so the streams are declared FIRST: they outlive every buffer and event.
struct rf_plan {
  // own_stream: `stream` unless rf_plan_set_stream gave another; comm_stream: the exchange of pipelined slab batches; dl_stream: the host
  // sink's device -> host copies; aux_stream: the MT19937 replays of rf_realise_batch_reference
  rfc::OwnedStream own_stream, comm_stream, dl_stream, aux_stream;
  hipStream_t stream = nullptr;
  int nx = 0, ny = 0, nz = 0, nzc = 0, f64 = 0, device = 0, nranks = 1, rank = 0;
  int nxl = 0, nzl = 0, kz0 = 0;          // this rank's x-slab height, kz-slab width and first kz plane
  rfc::DevBuf<> R;                        // receive buffer of the all-to-all (slab-path plans only)
  rfc::DevBuf<> W2, R2;                   // second buffer pair of pipelined slab batches
  rfc::Events pev;                        // ... and their events: fwd[2], exch[2], z[2]
  bool force_slab = false;                // single-rank plan routed through the slab pipeline (tests)
  int standin_read_pct = 100, standin_write_pct = 100;   // ... and the share of the blocks it reads / writes (rf_slab_set_exchange_standin_ex)
  int standin_wg = 0;                     // rf_slab_set_exchange_standin: workgroups of the copy kernel that stands in for the all-to-all of a rank without a communicator
  // RF_FLAG_EXCHANGE_CHUNKS: the rank's kz slab as `xchunks` sub-slabs of nzl / xchunks planes, each generated, x- and y-transformed
  // and SENT on its own, so that the exchange of sub-slab c runs under the forward passes of sub-slab c + 1 (queue_c2r).  Layout:
  // W = [chunk][nx][ny][nzl / xchunks]; R = [source rank][chunk][nxl][ny][nzl / xchunks], which is what the gathering z pass reads
  // anyway with nranks * xchunks segments per row
  int xchunks = 1;
  rfc::Events chunk_ev;                   // forward half of chunk c queued (no timing)
  bool replicate = false;                 // multi-rank plan without an exchange: every rank generates all of k space (see queue_x)
  // "direct" exchange: the y pass stores its output tiles straight into the receive buffers of the ranks that own
  // their x planes (rf_fft.h DirectColIO) -- peer-mapped pointers between processes (rf_comm_enable_direct), plain device pointers between
  // virtual ranks (rf_slab_link_direct) -- and one tiny all-reduce per realisation is the barrier between the peers' stores and the z pass
  bool direct = false;
  std::vector<void*> peer_R[2];           // host: every rank's R and R2 as THIS process addresses them ([rank] = its own)
  rfc::DevBuf<void*> peer_tab;            // device: [2 buffers][chunks][nranks] destination bases, shifted as DirectColIO wants them
  int peer_tab_chunks = 0;                // ... built for this many exchange chunks
  std::vector<void*> ipc_open;            // peer mappings this process opened (closed at destroy)
  bool direct_standin = false;            // rf_slab_set_direct_standin: the stores land in this rank's own buffers (no field comes out)
  int direct_overlap = 1;                 // batches: 1 = the storing y pass on the exchange stream beside the neighbours' x / z passes, 0 = everything on one stream
  ncclComm_t comm = nullptr;
  size_t csize = 8;                       // bytes per complex element
  rfc::DevBuf<> W;                        // [nx][ny][nz] real == [nx][ny][nz/2] complex (packed Nyquist)
  rfc::DevBuf<> K;                        // lazy: API-layout k-space [nx][ny][nz/2+1]
  // lazy: the x pass's TRANSPOSED intermediate [kz tile][ny][nx][tile width]: the x pass stores whole
  // contiguous tiles there and the y pass goes X -> W out of place.  xposed = the plan may use it (RF_FLAG_TRANSPOSED_INTERMEDIATE).
  rfc::DevBuf<> X;
  bool xposed = false;
  // y and z passes slab by slab of x planes: -1 = automatic (slabs of about the Infinity Cache's size),
  // 0 = whole-grid passes, > 0 = this many x planes per slab (RF_FLAG_YZ_SLAB_PLANES)
  int yz_slab = -1;
  // rf_set_host_sink: the NEXT single-rank realisation delivers its field to host memory slab by slab, each slab's device -> host copy
  // on dl_stream behind that slab's z pass while the GPU runs the next slab (generate.py:184-189,230 returns a host array: the copy is
  // 15 x the realisation)
  void* sink_host = nullptr;              // armed destination (one shot), RF_LAYOUT_DENSE / RF_LAYOUT_PADDED rows
  int sink_layout = 0;
  bool sink_delivered = false;            // the last armed call has delivered
  rfc::Events sink_ev;
  int yz_merge = 1;                       // rf_set_merged_yz: 0 never, 1 untimed calls (default), 2 timed calls too (a mark per launch)
  rfc::DevBuf<> P;                        // lazy: saved potential, API layout, at offset 0 of its allocation (ensure_p)
  size_t w_bytes = 0, k_bytes = 0, p_bytes = 0;      // field buffer, k-space side array, potential array (padded rows)
  int ppitch = 0;                         // cells per row of the potential array: nzl + 1, rounded up to even on float32 plans
  // lazy, rf_lpt2_source: the accumulators T and S of the real-space sweep (2 x w_bytes); once the source exists they are dead and the
  // same memory holds the second-order potential in P's padded layout (rf_lpt2_potential; p_bytes <= L.bytes).  has.potential2() goes
  // stale with everything that writes P or starts a new source.
  rfc::DevBuf<> L;
  // lazy, rf_particles_*: the particle displacements Q[3][nx][ny][nz] of the plan's real type (3 x w_bytes) and the 64-bit accumulator
  // grid A[nx][ny][nz] of the cloud-in-cell paint (8 bytes per cell), both counted by rf_plan_nbytes; pa_drop: the paint's counter of
  // dropped particles (8 bytes).  has.counts(): A holds the counts of a paint; paint_form: 0 auto, 1 global, 2 tiled.
  rfc::DevBuf<> Q, A, pa_drop;
  int paint_form = 0;
  // lazy, rf_particles_gather: the gathered values PG[3][nx][ny][nz] of the plan's real type (3 x w_bytes, zeroed once), indexed by the
  // particle's lattice cell as Q is and counted by rf_plan_nbytes; the drop counter is pa_drop.  gather_form: 0 auto, 1 global, 2 tiled.
  rfc::DevBuf<> PG;
  int gather_form = 0;
  // lazy, rf_kspace_stash: a second half spectrum of K's size and layout (k_bytes, counted by rf_plan_nbytes) -- the first grid's spectrum
  // of an interlaced paint; has.stash().  il_tab: the combine's three phase tables on the device, (nx + ny + nz/2 + 1) float64 pairs.
  rfc::DevBuf<> KS;
  rfc::DevBuf<double> il_tab;
  rfc::DevBuf<> tw_x, tw_y, tw_z;
  rfc::DevBuf<double> kx2, ky2, kz2;
  rfc::DevBuf<double> xt, st, sl;
  rfc::DevBuf<int> bin;
  int nt = 0, nbins = 0;
  double x0 = 0, inv_dx = 0;
  bool have_kgrid = false, have_power = false;
  // fast float32 native generation: float copies of the k^2 tables + per-bin sigma records
  rfc::DevBuf<rf::FastRec> frec;
  int fnbins = 0;
  float fdkx = 0, fdky = 0, fdkz = 0, fu_scale = 0, fu_off = 0;
  bool have_fast = false, exact_gen = false;
  std::vector<double> h_kx2, h_ky2, h_kz2;   // host copies (k range of the grid for the fast records)
  rf::SigmaTableHost h_tab;
  rfc::DevBuf<double> noise;              // has.deviates64(): a full set of deviates
  rfc::DevBuf<> fixbuf;                // nx * ny complex: the repaired kz = 0 slots of the fast generation pass (fix_fill_kernel)
  rfc::MtReplay mt;                    // the MT19937 replay (rf_noise_mt19937, rf_mt_share_*, rf_realise_batch_reference): table, buffers, step
  rfc::DevBuf<double> partials;
  long long npartials = 0;
  rfc::DevBuf<double> stats;              // (sum, sumsq) per realisation
  rfc::DevBuf<uint64_t> seeds_dev;
  // the caller's seed array may be a temporary: it is copied into one of two plan-owned pinned staging slots before
  // the asynchronous upload (a slot is reused only after the upload that last read it has completed)
  rfo::Buffer<rfc::HipPinned, uint64_t> seeds_pin[2];
  rfc::Events seeds_ev;
  int seeds_turn = 0;
  rfc::DevBuf<double> coll_scratch;       // 2 doubles on the device for host-side all-reduces (never aliases `stats`)
  rfc::DevBuf<double> ztab;               // 2 * nz doubles for lognormal / affine tables
  // fused lognormal realisations (rf_realise_lognormal): [growth nz][density nz][A nz][B nz][sigma 8] and the y pass's Parseval partials
  rfc::DevBuf<double> lntab, ypart;
  bool ln_tables = false, ln_density = false;
  rfc::Timeline tl;                    // the last call's start, end and marks: rf_elapsed_ms, rf_kernel_ms, rf_merged_yz_ms
  bool unpacked = false;               // c2c plan: W is the full [nx][ny][nz] complex array, only rf_*_c / rf_execute_c2c apply
  // non-power-of-two grid (rf_generic.h): the transforms run on API-layout arrays, K -> G -> W (generation fused into the x pass only
  // with fused_generic), no graphs, one rank.  gax / gay factor nx / ny, gaz factors nz/2 (packed plans) or nz (c2c plans)
  bool generic = false;
  rfc::DevBuf<> G;                     // lazy scratch [nx][ny][nz/2+1] complex (c2c plans: [nx][ny][nz], for a long axis)
  rfc::DevBuf<> G2;                    // lazy second scratch: only when an axis is too long for one line (four-step form, rf_generic.h)
  rf::GenericAxis gax, gay, gaz;
  rf::GenericDims gdims;               // the same + the split of the long axes, as the sequences of rf_generic.h take them
  bool fused_generic = false;          // RF_FLAG_FUSED_GENERIC_GENERATION: realisations generate inside the x pass (no K; has.kspace() untouched)
  rfc::DevBuf<> pw_buf;                 // lazy, rf_measure_power: squared edges, result, per-workgroup partials
  rfc::DevBuf<> mp_buf;                 // lazy, rf_measure_multipoles: squared edges, result, compensation tables, per-workgroup partials (counted by rf_plan_nbytes)
  // lazy, rf_measure_bispectrum (all counted by rf_plan_nbytes, freed by rf_bispectrum_release or with the plan): bs_mask, one masked half
  // spectrum (k_bytes); bs_fields, the nbins shell fields (w_bytes each) of the last call; bs_part: [squared edges, 33 slots][result,
  // 8192 slots][packed triples, 8192 words][amplitude tables: nx, ny, nz/2 + 1 slots][rows x ntriples partials].  bs_nbins: the shell
  // fields bs_fields holds (0: none); bs_max_wg: rf_bispectrum_set_max_workgroups (0: the launchers' own caps)
  rfc::DevBuf<> bs_mask, bs_fields, bs_part;
  int bs_nbins = 0, bs_max_wg = 0;
  struct BatchGraph { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
  std::map<int, BatchGraph> graphs;       // captured batch graphs, keyed by the number of realisations
  rfc::Contents has;                      // what W / W2, stats, K, noise / mt.scratch, L and A hold right now
};

namespace rfc {
// which pipeline the plan runs (rf_route.h), from the plan's facts as they are NOW: asked per question, never kept
inline Route route(const rf_plan* p) {
  RouteFacts f;
  f.unpacked = p->unpacked; f.generic = p->generic; f.nranks = p->nranks; f.force_slab = p->force_slab;
  f.replicate = p->replicate; f.direct = p->direct; f.xchunks = p->xchunks;
  return route_of(f);
}

// which generator fills an x pass of the plan (rf_source.h), from the plan's facts as they are at the moment of the call
inline SourceFacts source_facts(const rf_plan* p) {
  SourceFacts f;
  f.f64 = p->f64 != 0; f.have_fast = p->have_fast; f.exact_gen = p->exact_gen; f.kind = route(p).kind;
  f.deviates = p->has.deviates32() ? SourceFacts::Pairs32 : p->has.deviates64() ? SourceFacts::Float64 : SourceFacts::None;
  return f;
}
inline Source source(const rf_plan* p, const SourceAsk& ask) { return source_of(source_facts(p), ask); }
static_assert(SourceAsk::Native == RF_NOISE_NATIVE && SourceAsk::External == RF_NOISE_EXTERNAL && SourceAsk::Resident == RF_NOISE_RESIDENT, "noise modes");

// What ONE call asks of the passes it queues.  The entry point builds it on its stack and hands it down by const reference
// (queue_c2r ... queue_x / queue_yz / make_fast); a default-constructed one is a plain NATIVE realisation, or the transform of a given k-space array.  Nothing of it outlives the call.
struct CallDesc {
  explicit CallDesc(int noise_mode = RF_NOISE_NATIVE) : mode(noise_mode) {}
  int mode;                               // the noise mode as the API names it (RF_NOISE_RESIDENT: draw from the device-resident deviates)
  bool emit_potential = false;            // transform emit_pscale * delta(k) / k^2 instead of delta(k) (rf_realise_scaled_potential)
  double emit_pscale = 0.0;
  const double* zscale = nullptr;         // the z pass multiplies plane z by zscale[z] (device table: ztab)
  void* pot_target = nullptr;             // the x pass also stores delta(k) / k^2 there (rf_realise_potential)
  bool intermediate = false;              // the transform's output is an intermediate of the call, not the plan's field: no host sink delivery, no moments (rf_measure_bispectrum)
  // what the call's x pass asks of source(p, ...) (kspace: it transforms that array instead of generating)
  SourceAsk ask(bool kspace) const { return SourceAsk::x_pass(kspace, mode, emit_potential ? SourceAsk::Emitted : pot_target ? SourceAsk::Stored : SourceAsk::Nothing); }
};

// (defined in rf_capi.hip)
void drop_graphs(rf_plan* p);
int ensure_k(rf_plan* p);
int ensure_x(rf_plan* p);
int ensure_noise(rf_plan* p);
bool xpose_ok(const rf_plan* p);
GenParams make_gen(rf_plan* p, uint64_t seed, int mode);
int upload_noise(rf_plan* p, int mode, const double* noise_host);
int queue_x(rf_plan* p, const CallDesc& cd, const GenParams& gp, const void* kspace, void* W, hipStream_t sx, Timeline* tl, int kz0c = -1, int nzlc = -1);
int queue_xy(rf_plan* p, const CallDesc& cd, const GenParams& gp, const void* kspace, void* W, hipStream_t s, Timeline* tl, int rbuf = 0);
int ensure_batch_buffers(rf_plan* p);
int rebuild_peer_tab(rf_plan* p);
int direct_barrier(rf_plan* p, hipStream_t s);
int queue_yz(rf_plan* p, const CallDesc& cd, void* W, hipStream_t s, double* stats_out, Timeline* tl);
int ensure_stats(rf_plan* p, int n);
int rms_from_stats(rf_plan* p, int n, double* rms_out);
int queue_z_slab(rf_plan* p, const void* R, void* W, double* stats_out, hipStream_t s);
int queue_r2c_slab_rows(rf_plan* p, hipStream_t s);
int queue_r2c_slab_cols(rf_plan* p, hipStream_t s);
int queue_r2c_single(rf_plan* p, bool unpack, void* spectrum);
int potential_forward(rf_plan* p, uint64_t seed, int mode, const double* noise_host, bool whole);
}  // namespace rfc
