// rf_capi_mt.hip -- C-ABI entry points of the on-GPU replay of np.random.RandomState(seed).normal (random.py:24-28): the jump table,
// the replay (float64 / float32 pairs), the stream shared between the ranks of a kz-slab job, same-seed batches.  Kernels: rf_k_mt.hip.
#include "rf_plan.h"

using namespace rfc;

extern "C" {

int rf_mt_set_jump(rf_plan* p, int npolys, const uint16_t* pos, const int* npos, int stride, int blocks_per_segment, int radix) {
  RF_REQUIRE(p && pos && npos, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(npolys >= 1 && stride >= 1 && blocks_per_segment >= 1 && radix >= 2 && npolys % (radix - 1) == 0, "invalid jump table");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipStreamSynchronize(p->stream));
  RF_HIP(p->mt.pos.release());                    // (always fresh tables)
  RF_HIP(p->mt.npos_dev.release());
  const WideTable w = widen_jump_table(npolys, pos, npos, stride);
  RF_REFUSE(w.refusal);
  RF_HIP(p->mt.pos.reserve(w.rows.size() * sizeof(uint32_t)));
  RF_HIP(hipMemcpy(p->mt.pos.get(), w.rows.data(), w.rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  RF_HIP(p->mt.npos_dev.reserve(w.counts.size() * sizeof(int)));
  RF_HIP(hipMemcpy(p->mt.npos_dev.get(), w.counts.data(), w.counts.size() * sizeof(int), hipMemcpyHostToDevice));
  p->mt.table.npos.assign(npos, npos + npolys);
  p->mt.table.stride = w.wstride;
  p->mt.table.bps = blocks_per_segment;
  p->mt.table.radix = radix;
  return 0;
}

int rf_noise_mt19937(rf_plan* p, const uint32_t* state624, unsigned long long* accepted) {
  return rf_noise_mt19937_ex(p, state624, accepted, 0);
}

namespace {
// sizes of one replay of RandomState(seed).normal for this plan's grid (rf_replay.h), if the uploaded table reaches that far
int mt_geom(rf_plan* p, int single, ReplayGeom& g) {
  g = replay_geom((unsigned long long)p->nx * p->ny * (p->nzc + 1), p->mt.table.bps, p->mt.table.radix, single != 0);
  RF_REFUSE(p->mt.table.refuses(g));
  return 0;
}
bool pairs32_fit(const rf_plan* p, const ReplayGeom& g) { return pairs32_fit(g, p->nzc + 1); }
int mt_ensure_buffers(rf_plan* p, const ReplayGeom& g) {
  RF_HIP(p->mt.states.reserve((size_t)g.nseg * 624 * sizeof(uint32_t)));
  const size_t seg = ((size_t)g.nseg + 1) * sizeof(unsigned long long);
  if (p->mt.counts.bytes < seg || p->mt.offsets.bytes < seg) {      // the pair grows together: both freed, then both allocated
    RF_HIP(p->mt.counts.release());
    RF_HIP(p->mt.offsets.release());
  }
  RF_HIP(p->mt.counts.reserve(seg));
  RF_HIP(p->mt.offsets.reserve(seg));
  RF_HIP(p->mt.rowtab.reserve((size_t)p->nx * p->ny * sizeof(RowLoc)));
  RF_HIP(p->mt.flags.reserve(sizeof(int)));
  RF_HIP(p->mt.scratch.reserve(g.need));
  return 0;
}
// the jump tree over the first nseg states of p->mt.states (rf_replay.h for_each_tree_stage): one launch per stage
int mt_queue_tree(rf_plan* p, int nseg, hipStream_t s) {
  const MtReplay& mt = p->mt;
  const int R = mt.table.radix;
  return for_each_tree_stage(nseg, R, [&](int t, int nsrc, long long dist) -> int {
    RF_HIP(launch_mt_jump(mt.states.get(), mt.pos.get() + (size_t)t * (R - 1) * mt.table.stride, mt.npos_dev.get() + 4 * t * (R - 1), mt.table.stride, nsrc,
                          dist, R - 1, nseg, s));
    return 0;
  });
}
// the replay itself on stream s, from the start state in p->mt.states[0 .. 624): jump tree, ONE generation pass, scan (and the
// move into cell order for float64 deviates).  No host synchronisation.
int mt_queue(rf_plan* p, const ReplayGeom& g, int single, hipStream_t s) {
  if (int rc = mt_queue_tree(p, g.nseg, s)) return rc;
  // ONE generation pass: every segment writes its accepted pairs densely into its own run of the scratch array
  // (capacity = its attempts) and counts them; a scan of the counts gives each run its first cell, and a copy kernel
  // moves the runs into place.  (Round 1 generated every block twice -- a count pass, then a fill pass that knew the
  // offsets: 2.5 + 3.3 ms against 3.3 + 1.x ms for fill + move.)  A kz-slab rank replays the WHOLE stream (where a
  // deviate goes depends on every earlier acceptance) and keeps the deviates of its own planes while moving.
  RF_HIP(launch_mt_polar(single != 0, p->mt.states.get(), g.nseg, p->mt.table.bps, g.total_blocks, p->mt.counts.get(), p->mt.scratch.ptr, g.cap, s));
  RF_HIP(launch_mt_scan(p->mt.counts.get(), p->mt.offsets.get(), g.nseg, s));
  // float64 deviates are moved into cell order (and cut to this rank's planes); float32 ones stay in the segments' runs:
  // the generation pass finds cell c through the scan (slack_cell), which saves the 1.7 ms copy per 1024^3
  if (single) {
    RF_HIP(hipMemsetAsync(p->mt.flags.get(), 0, sizeof(int), s));
    RF_HIP(launch_mt_rowtab(p->mt.offsets.get(), g.nseg, p->mt.rowtab.ptr, p->nx, p->ny, (int)p->nzc + 1, p->mt.flags.get(), s));
  }
  if (!single)
    RF_HIP(launch_mt_compact(false, p->mt.scratch.ptr, p->mt.counts.get(), p->mt.offsets.get(), g.nseg, g.cap, p->noise.get(), g.ncells, (int)p->nzc + 1,
                             (int)p->nzl + 1, p->kz0, s));
  return 0;
}
}  // namespace

int rf_noise_mt19937_ex(rf_plan* p, const uint32_t* state624, unsigned long long* accepted, int single) {
  RF_REQUIRE(p && state624, "null argument");
  // `single` is a request: plans without the fast float32 generation pass (float64, generic shapes, exact-generation
  // flag, tables too dense for the per-bin records) read float64 deviates and get them
  if (single && !resident_reads_pairs32(source_facts(p))) single = 0;
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->mt.table_uploaded(), "rf_mt_set_jump must be called first");
  RF_HIP(hipSetDevice(p->device));
  if (!single)
    if (int rc = ensure_noise(p)) return rc;
  ReplayGeom g;
  if (int rc = mt_geom(p, single, g)) return rc;
  if (single && !pairs32_fit(p, g)) {
    single = 0;
    if (int rc = ensure_noise(p)) return rc;
    if (int rc = mt_geom(p, single, g)) return rc;
  }
  if (int rc = mt_ensure_buffers(p, g)) return rc;
  hipStream_t s = p->stream;
  RF_HIP(hipMemcpyAsync(p->mt.states.get(), state624, 624 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  if (int rc = mt_queue(p, g, single, s)) return rc;
  const int nseg = g.nseg;
  unsigned long long total = 0;
  int flags = 0;
  p->has.deviates_none();
  RF_HIP(hipMemcpyAsync(&total, p->mt.offsets.get() + nseg, sizeof(total), hipMemcpyDeviceToHost, s));
  if (single) RF_HIP(hipMemcpyAsync(&flags, p->mt.flags.get(), sizeof(flags), hipMemcpyDeviceToHost, s));
  RF_HIP(hipStreamSynchronize(s));
  p->mt.nseg = nseg;
  p->mt.seg_cap = g.cap;
  if (accepted) *accepted = total;
  RF_REQUIRE(total >= g.ncells, "MT19937 replay: not enough accepted polar attempts (increase the margin)");
  RF_REQUIRE(!(flags & 1), "MT19937 replay: a segment holds fewer deviate pairs than a row of the grid has cells (segment length too short for the float32 form)");
  if (!single) {
    p->has.deviates64_ready();
    // the runs are dead once the compaction has moved them into p->noise (the stream is idle here).  They are 1.27x the noise
    // buffer -- 11 GB at 1024^3, the difference between fitting and not fitting a 2048^3 float64 plan with a saved potential
    // into 288 GB -- so they are given back when the device is getting full; otherwise they stay for the next seed (allocating
    // and releasing 11 GB costs ~0.5 s per call, a hundred times the replay).  (float32 deviates live IN the runs and keep them.)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < total_b / 3) {
      RF_HIP(p->mt.scratch.release());
    }
  } else p->has.deviates32_ready();
  return 0;
}

/* ---- one stream, P ranks: the replay of RandomState(seed).normal shared between the ranks of a kz-slab job -----------------
 * rf_noise_mt19937_ex on a multi-rank plan replays the WHOLE stream on every rank (where a deviate goes depends on every
 * earlier acceptance).  Here rank r replays only segments [r nseg / P, (r + 1) nseg / P): (1) rf_mt_share_begin jumps to its first
 * segment (one jump per radix-16 digit), grows the local tree, runs the generation pass and returns its per-segment counts; (2) the
 * host gathers all counts (a few thousand integers) and hands them to rf_mt_share_pack, which scans them -- now every rank knows
 * which cells every rank holds -- and packs the local pairs by destination (kz slab); (3) ONE all-to-all of deviates, 8 B per
 * cell in float32 mode: the same volume as the field's exchange (rf_mt_share_exchange over RCCL, or rf_mt_share_exchange_local
 * between virtual ranks on one device); (4) rf_mt_share_finish leaves them as the plan's resident float64 deviates, the form
 * rf_realise(RF_NOISE_RESIDENT) and the other consumers already read on multi-rank plans.  Per rank: 1/P of the replay's time
 * and of its scratch.  float64 mode moves the exact deviates (16 B per cell) and gives bit for bit what the replicated
 * replay gives; float32 mode (complex64 plans) rounds the Box-Muller factor as rf_noise_mt19937_ex(single = 1) does. */
int rf_mt_share_segments(rf_plan* p, int* nseg_total, int* seg_first, int* seg_count) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked && !p->generic, "the distributed replay serves packed plans on the tiled kernels");
  RF_REQUIRE(p->mt.table_uploaded(), "rf_mt_set_jump must be called first");
  ReplayGeom g;
  if (int rc = mt_geom(p, 1, g)) return rc;
  const int a = sh_seg_begin(p->rank, g.nseg, p->nranks), b = sh_seg_begin(p->rank + 1, g.nseg, p->nranks);
  if (nseg_total) *nseg_total = g.nseg;
  if (seg_first) *seg_first = a;
  if (seg_count) *seg_count = b - a;
  return 0;
}

int rf_mt_share_begin(rf_plan* p, const uint32_t* state624, int single, unsigned long long* counts_out) {
  RF_REQUIRE(p && state624 && counts_out, "null argument");
  RF_REQUIRE(!p->unpacked && !p->generic, "the distributed replay serves packed plans on the tiled kernels");
  RF_REQUIRE(!route(p).replicates(), "replicated-generation plans draw native deviates only");
  RF_REQUIRE(p->mt.table_uploaded(), "rf_mt_set_jump must be called first");
  RF_REQUIRE(p->nranks >= 1 && p->nranks <= 64, "unsupported number of ranks");
  if (single && p->f64) single = 0;                      // float64 cells: keep the exact deviates
  RF_HIP(hipSetDevice(p->device));
  p->mt.step.reset();
  if (int rc = ensure_noise(p)) return rc;
  ReplayGeom g;
  if (int rc = mt_geom(p, single, g)) return rc;
  const int first = sh_seg_begin(p->rank, g.nseg, p->nranks), nloc = sh_seg_begin(p->rank + 1, g.nseg, p->nranks) - first;
  RF_REQUIRE(nloc >= 1, "more ranks than segments: use rf_noise_mt19937_ex on this grid");
  ReplayGeom gl = g;
  gl.nseg = nloc + kSpareSlots;                           // + slots for the jump to the first segment
  gl.need = (size_t)nloc * g.cap * (single ? 2 * sizeof(float) : 2 * sizeof(double));
  if (int rc = mt_ensure_buffers(p, gl)) return rc;
  hipStream_t s = p->stream;
  MtReplay& mt = p->mt;
  // the start state of segment `first`: hop by hop through the spare slots behind the local states (rf_replay.h digit_hops)
  int slot = nloc;
  RF_HIP(hipMemcpyAsync(mt.states.get() + (size_t)slot * 624, state624, 624 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  const Hops hops = digit_hops(first, mt.table.radix, g.stages);
  RF_REFUSE(hops.refusal);
  for (int i = 0; i < hops.n; ++i, ++slot) {
    const int row = hops.rows[i];
    RF_HIP(launch_mt_jump(mt.states.get() + (size_t)slot * 624, mt.pos.get() + (size_t)row * mt.table.stride, mt.npos_dev.get() + 4 * row, mt.table.stride,
                          1, 1, 1, 2, s));
  }
  RF_HIP(hipMemcpyAsync(mt.states.get(), mt.states.get() + (size_t)slot * 624, 624 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  // the local tree and the generation pass over the local segments
  if (int rc = mt_queue_tree(p, nloc, s)) return rc;
  RF_HIP(launch_mt_polar(single != 0, mt.states.get(), nloc, mt.table.bps, g.total_blocks - (long long)first * mt.table.bps, mt.counts.get(), mt.scratch.ptr, g.cap, s));
  RF_HIP(hipMemcpyAsync(counts_out, mt.counts.get(), (size_t)nloc * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  RF_HIP(hipStreamSynchronize(s));
  mt.sh_first = first; mt.sh_nloc = nloc;
  p->has.deviates_none();                                 // (p->noise is about to be overwritten; the runs in mt.scratch are this rank's share only)
  mt.step.replay_done(single != 0);
  return 0;
}

// every rank's per-segment counts, in segment order, on every rank: an integer sum over the communicator of arrays that are zero
// outside the rank's own range (a few thousand values; also the first collective after the local replays)
int rf_mt_share_gather(rf_plan* p, unsigned long long* counts_all) {
  RF_REQUIRE(p && counts_all, "null argument");
  RF_REFUSE(p->mt.step.refuses_gather());
  RF_REQUIRE(p->nranks == 1 || p->comm != nullptr, "rf_comm_init has not been called on this multi-rank plan");
  RF_HIP(hipSetDevice(p->device));
  ReplayGeom g;
  if (int rc = mt_geom(p, p->mt.step.single(), g)) return rc;
  if (p->comm_stream) RF_HIP(hipStreamSynchronize(p->comm_stream));          // (the communicator is used from one stream at a time)
  DevBuf<unsigned long long> tmp_buf;
  RF_HIP(tmp_buf.reserve((size_t)g.nseg * sizeof(unsigned long long)));
  unsigned long long* tmp = tmp_buf.get();
  hipStream_t s = p->stream;
  hipError_t e = hipMemsetAsync(tmp, 0, (size_t)g.nseg * sizeof(unsigned long long), s);
  if (e == hipSuccess) e = hipMemcpyAsync(tmp + p->mt.sh_first, p->mt.counts.get(), (size_t)p->mt.sh_nloc * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && p->comm && g_rccl.AllReduce(tmp, tmp, (size_t)g.nseg, ncclUint64, ncclSum, p->comm, s) != ncclSuccess) e = hipErrorUnknown;
  if (e == hipSuccess) e = hipMemcpyAsync(counts_all, tmp, (size_t)g.nseg * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  RF_HIP(e);
  return 0;
}

int rf_mt_share_pack(rf_plan* p, const unsigned long long* counts_all) {
  RF_REQUIRE(p && counts_all, "null argument");
  RF_REFUSE(p->mt.step.refuses_pack());
  RF_HIP(hipSetDevice(p->device));
  MtReplay& mt = p->mt;
  const bool single = mt.step.single();
  ReplayGeom g;
  if (int rc = mt_geom(p, single, g)) return rc;
  const int P = p->nranks, nzl = (int)p->nzl, nzh = (int)p->nzc + 1;
  ShareSplit split = share_split(counts_all, g, P, p->rank, nzl, nzh);
  RF_REFUSE(split.refusal);
  mt.split = std::move(split);
  const size_t es = single ? 2 * sizeof(float) : 2 * sizeof(double);
  const size_t send_bytes = (size_t)(mt.split.sendoff[P] > 0 ? mt.split.sendoff[P] : 1) * es;
  const size_t recv_pairs = (size_t)p->nx * p->ny * (nzl + 1);
  if (mt.send.bytes < send_bytes) RF_HIP(mt.send.reserve(send_bytes + send_bytes / 64));    // (the shares differ from seed to seed by the counts' binomial noise)
  if (single) RF_HIP(mt.recv.reserve(recv_pairs * es));
  RF_HIP(mt.sbase.reserve(64 * sizeof(long long)));
  RF_HIP(mt.first.reserve((size_t)mt.sh_nloc * sizeof(unsigned long long)));
  hipStream_t s = p->stream;
  RF_HIP(hipMemcpyAsync(mt.sbase.get(), mt.split.sbase.data(), (size_t)P * sizeof(long long), hipMemcpyHostToDevice, s));
  RF_HIP(hipMemcpyAsync(mt.first.get(), mt.split.first.data() + mt.sh_first, (size_t)mt.sh_nloc * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  RF_HIP(launch_mt_share_pack(single, mt.scratch.ptr, mt.counts.get(), mt.first.get(), mt.sh_nloc, g.cap, mt.send.ptr, g.ncells, nzh, nzl, P,
                              mt.sbase.get(), s));
  RF_HIP(hipStreamSynchronize(s));                        // (the uploads read host memory)
  mt.step.pack_done();
  return 0;
}

namespace {
// where rank p's stream arrives: the resident deviates themselves (float64) or the float32 staging buffer
inline char* sh_recv_base(rf_plan* p) { return p->mt.step.single() ? (char*)p->mt.recv.ptr : (char*)p->noise.get(); }
}

int rf_mt_share_exchange(rf_plan* p) {
  RF_REQUIRE(p, "null plan");
  RF_REFUSE(p->mt.step.refuses_exchange());
  RF_REQUIRE(p->nranks == 1 || p->comm != nullptr, "rf_comm_init has not been called on this multi-rank plan");
  RF_HIP(hipSetDevice(p->device));
  const size_t es = p->mt.step.single() ? 2 * sizeof(float) : 2 * sizeof(double);
  hipStream_t s = p->stream;
  const int me = p->rank;
  const ShareSplit& sp = p->mt.split;
  RF_HIP(hipMemcpyAsync(sh_recv_base(p) + sp.recvoff[me] * es, (const char*)p->mt.send.ptr + sp.sendoff[me] * es, sp.sendcnt[me] * es, hipMemcpyDeviceToDevice, s));
  if (p->nranks > 1) {
    RF_NCCL(g_rccl.GroupStart());
    for (int h = 0; h < p->nranks; ++h) {
      if (h == me) continue;
      if (sp.sendcnt[h]) RF_NCCL(g_rccl.Send((const char*)p->mt.send.ptr + sp.sendoff[h] * es, sp.sendcnt[h] * es, ncclUint8, h, p->comm, s));
      if (sp.recvcnt[h]) RF_NCCL(g_rccl.Recv(sh_recv_base(p) + sp.recvoff[h] * es, sp.recvcnt[h] * es, ncclUint8, h, p->comm, s));
    }
    RF_NCCL(g_rccl.GroupEnd());
  }
  p->mt.step.exchange_done();
  return 0;
}

int rf_mt_share_exchange_local(rf_plan** plans, int n) {
  RF_REQUIRE(plans && n >= 1, "null argument");
  for (int g = 0; g < n; ++g) {
    RF_REQUIRE(plans[g] && plans[g]->nranks == n && plans[g]->rank == g, "plans must be ranks 0..n-1 of one n-rank job");
    RF_REQUIRE(plans[g]->device == plans[0]->device, "virtual ranks must live on one device");
    RF_REFUSE(plans[g]->mt.step.refuses_exchange_local(plans[0]->mt.step));
    RF_HIP(hipStreamSynchronize(plans[g]->stream));
  }
  const size_t es = plans[0]->mt.step.single() ? 2 * sizeof(float) : 2 * sizeof(double);
  for (int g = 0; g < n; ++g)        // sender g, receiver h
    for (int h = 0; h < n; ++h) {
      RF_REQUIRE(plans[g]->mt.split.sendcnt[h] == plans[h]->mt.split.recvcnt[g], "send / receive counts disagree");
      if (plans[g]->mt.split.sendcnt[h])
        RF_HIP(hipMemcpy(sh_recv_base(plans[h]) + plans[h]->mt.split.recvoff[g] * es, (const char*)plans[g]->mt.send.ptr + plans[g]->mt.split.sendoff[h] * es,
                         plans[g]->mt.split.sendcnt[h] * es, hipMemcpyDeviceToDevice));
    }
  RF_HIP(hipDeviceSynchronize());       // (see rf_slab_exchange_local)
  for (int g = 0; g < n; ++g) plans[g]->mt.step.exchange_done();
  return 0;
}

int rf_mt_share_finish(rf_plan* p, unsigned long long* accepted) {
  RF_REQUIRE(p, "null plan");
  RF_REFUSE(p->mt.step.refuses_finish());
  RF_HIP(hipSetDevice(p->device));
  if (p->mt.step.single())
    RF_HIP(launch_mt_share_widen(p->mt.recv.ptr, p->noise.get(), (long long)p->nx * p->ny * (p->nzl + 1), p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  p->has.deviates64_ready();
  p->mt.step.finish_done();
  if (accepted) *accepted = p->mt.split.total;
  return 0;
}

// Same-seed realisations back to back (random.py:24-28 for n seeds): the replay of seed i + 1 (VALU / LDS-bound, second stream)
// runs under the y and z passes of seed i (HBM-bound); ONE set of runs -- the replay of seed i + 1 starts when the generation
// pass of seed i has read them, the generation pass of seed i + 1 when the replay has finished.  complex64 plans with the fast
// generation path (float32 pairs).  states: n x 624 words (mt19937.seed_state); rms_out: n, optional.
int rf_realise_batch_reference(rf_plan* p, const uint32_t* states, int n, double* rms_out) {
  RF_REQUIRE(p && states, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(n >= 1, "need at least one seed");
  RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
  RF_REQUIRE(p->mt.table_uploaded(), "rf_mt_set_jump must be called first");
  RF_REQUIRE(route(p).single() && resident_reads_pairs32(source_facts(p)),
             "rf_realise_batch_reference is for single-GPU complex64 plans on the fast generation path; loop rf_noise_mt19937 + rf_realise otherwise");
  RF_HIP(hipSetDevice(p->device));
  ReplayGeom g;
  if (int rc = mt_geom(p, 1, g)) return rc;
  RF_REQUIRE(pairs32_fit(p, g), "the replay's segments are too short for the float32 form on this grid: loop rf_noise_mt19937 + rf_realise");
  if (int rc = mt_ensure_buffers(p, g)) return rc;
  if (int rc = ensure_x(p)) return rc;
  RF_HIP(hipStreamSynchronize(p->stream));
  if (int rc = ensure_stats(p, n)) return rc;
  RF_HIP(p->aux_stream.create(hipStreamNonBlocking));
  RF_HIP(p->mt.bev.ensure(2, hipEventDisableTiming));
  // all start states and the per-seed accepted totals live on the device for the length of the batch (the plan keeps the block)
  if (p->mt.br_cap < n) {                                    // (br_cap: the block's layout is computed from it)
    p->mt.br_cap = 0;
    RF_HIP(p->mt.br_tmp.release());
    const int cap = n > 16 ? n : 16;
    RF_HIP(p->mt.br_tmp.reserve((size_t)cap * (624 * sizeof(uint32_t) + sizeof(unsigned long long) + sizeof(int) + 4)));
    p->mt.br_cap = cap;
  }
  uint32_t* dstates = (uint32_t*)p->mt.br_tmp.ptr;
  unsigned long long* dtotals = (unsigned long long*)((char*)p->mt.br_tmp.ptr + (size_t)p->mt.br_cap * 624 * sizeof(uint32_t));
  int* dflags = (int*)(dtotals + p->mt.br_cap);
  RF_HIP(hipMemcpy(dstates, states, (size_t)n * 624 * sizeof(uint32_t), hipMemcpyHostToDevice));
  hipStream_t S = p->stream, R = p->aux_stream;
  // whatever deviates were resident are about to be overwritten; the plan claims the new ones (and a field) only once every
  // replay of the batch has been checked
  p->has.deviates_none();
  p->has.field_consumed();
  p->mt.nseg = g.nseg;
  p->mt.seg_cap = g.cap;
  // both streams are drained before any return from here on
  auto drain = [&](int rc) { (void)hipStreamSynchronize(R); (void)hipStreamSynchronize(S); return rc; };
  auto replay = [&](int i) -> int {
    RF_HIP(hipMemcpyAsync(p->mt.states.get(), dstates + (size_t)i * 624, 624 * sizeof(uint32_t), hipMemcpyDeviceToDevice, R));
    if (int r = mt_queue(p, g, 1, R)) return r;
    RF_HIP(hipMemcpyAsync(dtotals + i, p->mt.offsets.get() + g.nseg, sizeof(unsigned long long), hipMemcpyDeviceToDevice, R));
    RF_HIP(hipMemcpyAsync(dflags + i, p->mt.flags.get(), sizeof(int), hipMemcpyDeviceToDevice, R));
    RF_HIP(hipEventRecord(p->mt.bev[0], R));
    return 0;
  };
  const CallDesc cd(RF_NOISE_RESIDENT);
  auto issue = [&]() -> int {
    RF_HIP(p->tl.begin(S, false));
    RF_HIP(hop(p->mt.bev[1], S, R));                         // (whatever ran on the main stream before the batch has finished with the runs)
    if (int rc = replay(0)) return rc;
    for (int i = 0; i < n; ++i) {
      RF_HIP(hipStreamWaitEvent(S, p->mt.bev[0], 0));        // the runs of seed i are complete
      p->has.deviates32_ready();                          // (queue_x selects the float32-pair kernel by it; cleared again on failure)
      const bool xp = p->X.ptr && xpose_ok(p);
      if (int rc = queue_x(p, cd, make_gen(p, 0, RF_NOISE_RESIDENT), nullptr, xp ? p->X.ptr : p->W.ptr, S, nullptr)) return rc;
      RF_HIP(hipEventRecord(p->mt.bev[1], S));               // the generation pass of seed i has read the runs
      if (i + 1 < n) {
        RF_HIP(hipStreamWaitEvent(R, p->mt.bev[1], 0));
        if (int rc2 = replay(i + 1)) return rc2;
      }
      if (int rc3 = queue_yz(p, cd, p->W.ptr, S, p->stats.get() + 2 * i, nullptr)) return rc3;
    }
    RF_HIP(p->tl.end(S));
    return 0;
  };
  std::vector<unsigned long long> totals((size_t)n);
  std::vector<int> flags((size_t)n);
  std::vector<double> rms((size_t)n);                      // (handed out only once every replay has been checked)
  int rc = issue();
  if (!rc) {
    hipError_t e = hipStreamSynchronize(R);
    if (e != hipSuccess) rc = fail(2, std::string("rf_realise_batch_reference: ") + hipGetErrorString(e));
  }
  if (!rc) rc = rms_from_stats(p, n, rms.data());          // (waits for S)
  if (!rc) {
    hipError_t e = hipMemcpy(totals.data(), dtotals, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(flags.data(), dflags, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(2, std::string("rf_realise_batch_reference: ") + hipGetErrorString(e));
  }
  if (!rc)
    for (int i = 0; i < n && !rc; ++i) {
      if (totals[i] < g.ncells) rc = fail(1, "MT19937 replay: not enough accepted polar attempts (increase the margin)");
      else if (flags[i] & 1) rc = fail(1, "MT19937 replay: a segment holds fewer deviate pairs than a row of the grid has cells");
    }
  if (rc) {
    p->has.deviates_none();
    return drain(rc);
  }
  p->has.deviates32_ready();                              // the last seed's deviates, as float32 pairs in the runs
  p->has.field_ready(p->W.ptr, n - 1);
  p->has.kspace_consumed();
  if (rms_out) memcpy(rms_out, rms.data(), (size_t)n * sizeof(double));
  return 0;
}

int rf_can_batch_reference(rf_plan* p) {
  if (!p || !route(p).single() || !resident_reads_pairs32(source_facts(p)) || !p->have_kgrid || !p->have_power || !p->mt.table_uploaded())
    return 0;
  ReplayGeom g;
  if (mt_geom(p, 1, g)) return 0;
  return pairs32_fit(p, g) ? 1 : 0;
}

int rf_download_noise(rf_plan* p, double* host, unsigned long long first, unsigned long long count) {
  RF_REQUIRE(p && host, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->has.deviates64(), "no float64 deviates resident on the device");
  RF_REQUIRE(first + count <= 2ull * p->nx * p->ny * (p->nzl + 1), "range outside the noise buffer");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(host, p->noise.get() + first, count * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}
}  // extern "C"
