// rf_capi.hip -- the C-ABI of include/randomfield_hip.h: plan object, device buffers, stream / graph orchestration of the HIP kernels
// (plans, inputs, realisations, transforms, host <-> device, timing; the replay of numpy's stream: rf_capi_mt.hip; the communicator
// and the slab pipeline step by step: rf_capi_slab.hip; shared helpers: rf_plan.h).
#include "rf_plan.h"

using namespace rf;
using namespace rfc;

namespace rfc {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

Rccl g_rccl;

int load_rccl() {
  if (g_rccl.lib) return 0;
  // If an RCCL is already in the process (e.g. the one bundled with PyTorch, which comes with its own HIP /
  // HSA runtime) it must be THAT one: a second librccl would talk to a second, uninitialised HSA runtime.
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
  void* h = nullptr;
  for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (h) break; }
  if (!h)
    for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
  if (!h) return fail(4, std::string("cannot load librccl: ") + dlerror());
#define RF_SYM(field, name)                                                        \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name));         \
  if (!g_rccl.field) return fail(4, std::string("librccl lacks ") + name);
  RF_SYM(GetUniqueId, "ncclGetUniqueId")
  RF_SYM(CommInitRank, "ncclCommInitRank")
  RF_SYM(CommDestroy, "ncclCommDestroy")
  RF_SYM(CommCount, "ncclCommCount")
  RF_SYM(GroupStart, "ncclGroupStart")
  RF_SYM(GroupEnd, "ncclGroupEnd")
  RF_SYM(Send, "ncclSend")
  RF_SYM(Recv, "ncclRecv")
  RF_SYM(AllReduce, "ncclAllReduce")
  RF_SYM(AllGather, "ncclAllGather")
  RF_SYM(GetErrorString, "ncclGetErrorString")
#undef RF_SYM
  g_rccl.lib = h;
  return 0;
}


void drop_graphs(rf_plan* p) {
  for (auto& kv : p->graphs) {
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
  }
  p->graphs.clear();
}

int ensure_k(rf_plan* p) { RF_HIP(p->K.reserve(p->k_bytes)); return 0; }

// is the stream inside a graph capture?  (no allocation and no host wait there)
bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

// numpy's normalisation of an inverse transform of the plan's grid
double inv_cells(const rf_plan* p) { return 1.0 / ((double)p->nx * (double)p->ny * (double)p->nz); }

// The saved potential is written by a second store stream of the generation pass, row for row next to the field's.  The time of
// that pass is bimodal -- 5.2 or 5.75 ms for the whole default call at 1024^3 -- and tools/pot_offset.py shows what decides it:
// NOT the virtual addresses (45 plans at identical virtual addresses of both arrays and 15 offsets of the potential inside its
// allocation, 256 B ... 4 MiB: either mode at every offset, the same offset in both modes) but the physical pages the driver
// happens to back them with, which user space neither sees nor chooses: the array sits at offset 0 of its allocation.
int ensure_p(rf_plan* p) { RF_HIP(p->P.reserve(p->p_bytes)); return 0; }

int ensure_g(rf_plan* p) { RF_HIP(p->G.reserve(p->k_bytes)); return 0; }

// May the plan hand the x pass's output to the y and z passes through the blocked intermediate X (rf_fft.h xblock_*_geom)?
// Single-rank tiled plans whose x and y passes use tiles of the same width, whose kz runs are whole tiles and whose z pass
// can gather (whole workgroups per x block and iy, whole segments per thread group).
int xpose_row_block(const rf_plan* p) { return col_gen_row_block(p->f64, p->nx, 64); }      // x rows per block of the transposed intermediate
bool xpose_ok(const rf_plan* p) {
  if (!p->xposed || !route(p).single()) return false;
  return xpose_shape_ok(p->f64, p->nx, p->ny, p->nzl, p->nzc, xpose_row_block(p));
}
int ensure_x(rf_plan* p) {
  if (xpose_ok(p)) RF_HIP(p->X.reserve(p->w_bytes));
  return 0;
}

// Any even shape (transform.py:172-177 asks for even axes, nothing more) whose axes either fit one line of the LDS
// (generic_max_axis(dtype): 8192 for complex64, 4096 for complex128) or split into two factors that do (the four-step form of
// rf_generic.h: up to cap^2).  packed: the contiguous axis is transformed at length nz / 2 (c2r / r2c plans), else at nz (c2c plans).
bool generic_dims(int nx, int ny, int nz, int f64, bool packed, GenericDims& d) {
  if (nx < 2 || ny < 2 || nz < 2 || (nx & 1) || (ny & 1) || (nz & 1)) return false;
  const int cap = generic_max_axis(f64);
  d = GenericDims();
  d.nx = nx; d.ny = ny; d.nz = nz; d.csize = f64 ? 16 : 8;
  // (a strided line that fits, but only one or two to a workgroup, runs the four-step form if its length splits: rf_generic.h generic_axis_form)
  auto one = [&](long long n, GenericAxis& ax, GenericLong& lg, bool strided) { return generic_axis_form(n, cap, (int)d.csize, strided, ax, lg); };
  // (a packed plan's root table of the contiguous axis has nz entries; nz itself must stay addressable: nz / 2 <= cap^2 is the limit that bites)
  return one(nx, d.ax, d.lx, true) && one(ny, d.ay, d.ly, true) && one(packed ? nz / 2 : nz, d.az, d.lz, false);
}
bool generic_shape(int nx, int ny, int nz, int f64, GenericAxis& ax, GenericAxis& ay, GenericAxis& az_half) {
  GenericDims d;
  if (!generic_dims(nx, ny, nz, f64, true, d)) return false;
  ax = d.ax; ay = d.ay; az_half = d.az;
  return true;
}

GenParams make_gen(rf_plan* p, uint64_t seed, int mode) {
  GenParams g;
  g.nx = p->nx; g.ny = p->ny; g.nz = p->nz;
  g.kx2 = p->kx2.get(); g.ky2 = p->ky2.get(); g.kz2 = p->kz2.get();
  g.xt = p->xt.get(); g.st = p->st.get(); g.sl = p->sl.get(); g.bin = p->bin.get();
  g.nt = p->nt; g.nbins = p->nbins; g.x0 = p->x0; g.inv_dx = p->inv_dx;
  g.noise_mode = (mode == RF_NOISE_RESIDENT) ? (int)RF_NOISE_EXTERNAL : mode; g.seed = seed; g.seed_dev = nullptr;   // graph batches point seed_dev at seeds_dev[i]
  g.noise = p->noise.get();
  g.zpitch = p->nzl + 1; g.zoff = p->kz0;      // side arrays (noise, K, P) hold this rank's planes + the Nyquist plane
  return g;
}

int ensure_noise(rf_plan* p) {
  const size_t need = 2 * (size_t)p->nx * p->ny * (p->nzl + 1) * sizeof(double);       // this rank's planes + the Nyquist plane
  if (p->noise.bytes < need) p->has.deviates64_dropped();
  RF_HIP(p->noise.reserve(need));
  return 0;
}

int upload_noise(rf_plan* p, int mode, const double* noise_host) {
  if (mode == RF_NOISE_RESIDENT) {
    RF_REQUIRE(p->has.deviates(), "no deviates resident on the device: call rf_noise_mt19937 (or an external-noise run) first");
    return 0;
  }
  if (mode != RF_NOISE_EXTERNAL) return 0;
  RF_REQUIRE(noise_host != nullptr, "external noise mode needs a host noise array");
  if (int rc = ensure_noise(p)) return rc;
  // the host array is the reference's full set, 2 doubles per cell of [nx][ny][nz/2+1]; a kz-slab rank keeps its own
  // planes and the Nyquist plane (one rank: everything, one contiguous copy)
  const size_t cell = 2 * sizeof(double), hp = (size_t)(p->nzc + 1) * cell, dp = (size_t)(p->nzl + 1) * cell, rows = (size_t)p->nx * p->ny;
  if (p->nranks == 1) {
    RF_HIP(hipMemcpyAsync(p->noise.get(), noise_host, rows * hp, hipMemcpyHostToDevice, p->stream));
  } else {
    RF_HIP(hipMemcpy2DAsync(p->noise.get(), dp, (const char*)noise_host + (size_t)p->kz0 * cell, hp, (size_t)p->nzl * cell, rows, hipMemcpyHostToDevice, p->stream));
    RF_HIP(hipMemcpy2DAsync((char*)p->noise.get() + (size_t)p->nzl * cell, dp, (const char*)noise_host + (size_t)p->nzc * cell, hp, cell, rows, hipMemcpyHostToDevice, p->stream));
  }
  p->has.deviates64_ready();
  return 0;
}

FastGenParams make_fast(rf_plan* p, const CallDesc& cd, uint64_t seed, bool seed_from_dev, const uint64_t* seed_ptr) {
  FastGenParams f;
  f.nx = p->nx; f.ny = p->ny; f.nz = p->nz;
  f.dkx = p->fdkx; f.dky = p->fdky; f.dkz = p->fdkz;
  f.rec = p->frec.get(); f.nbins = p->fnbins; f.u_scale = p->fu_scale; f.u_off = p->fu_off;
  f.seed = seed; f.seed_dev = seed_from_dev ? seed_ptr : nullptr;
  f.noise = nullptr; f.noise32 = nullptr;
  f.rowtab = nullptr; f.seg_cap = 0;
  f.zpitch = p->nzl + 1; f.zoff = p->kz0; f.ppitch = p->ppitch;
  f.pscale = cd.emit_pscale; f.emit_potential = cd.emit_potential ? 1 : 0;
  return f;
}

// (re)build the fast-path records once both the k grid and the power table are known
int build_fast(rf_plan* p) {
  // captured batch graphs carry the generation parameters (table pointers, bin scalars) by value: they are stale now
  RF_HIP(hipStreamSynchronize(p->stream));
  drop_graphs(p);
  p->have_fast = false;
  if (!p->have_kgrid || !p->have_power || p->generic) return 0;
  if (!col_fastgen_supported(p->f64, p->nx)) return 0;   // e.g. float64, nx = 2048: the exact kernel is used
  double kmax2 = 0, kmin2 = 1e300;
  auto scan = [&](const std::vector<double>& a) { for (double v : a) if (v > 0 && v < kmin2) kmin2 = v; };
  scan(p->h_kx2); scan(p->h_ky2); scan(p->h_kz2);
  auto mx = [](const std::vector<double>& a) { double m = 0; for (double v : a) m = v > m ? v : m; return m; };
  kmax2 = mx(p->h_kx2) + mx(p->h_ky2) + mx(p->h_kz2);
  if (!(kmin2 < 1e300) || !(kmax2 > 0)) return 0;
  std::vector<FastRec> rec;
  double x0, dx;
  if (!build_fast_records(p->h_tab, 0.5 * std::log10(kmin2) - 0.01, 0.5 * std::log10(kmax2) + 0.01, rec, x0, dx))
    return 0;   // knots too dense for the per-bin records: the exact kernel is used instead
  if ((int)rec.size() > FAST_LDS_BINS) return 0;   // the records must fit the kernel's LDS table
  // the fast kernel forms |k|^2 arithmetically, k_axis(i) = dk_axis * signed index: needs uniform fftfreq-style axes
  // (powertools.py:27-37 always makes them so); anything else keeps the exact kernel, which reads the tables
  auto regular = [](const std::vector<double>& a, int n, bool half, float& dk) {
    if (n < 2 || (int)a.size() < 2 || !(a[1] > 0)) return false;
    for (int i = 0; i < (int)a.size(); ++i) {
      const double j = (half || i < n / 2) ? i : i - n;
      const double want = j * j * a[1];
      if (std::fabs(a[i] - want) > 1e-9 * (want + 1e-300)) return false;
    }
    dk = (float)std::sqrt(a[1]);
    return true;
  };
  if (!regular(p->h_kx2, p->nx, false, p->fdkx) || !regular(p->h_ky2, p->ny, false, p->fdky) ||
      !regular(p->h_kz2, p->nz, true, p->fdkz))
    return 0;
  p->fu_scale = (float)(0.5 * std::log10(2.0) / dx);
  p->fu_off = (float)(-x0 / dx);
  RF_HIP(p->frec.release());                    // (always a fresh table, as long as the new records)
  RF_HIP(p->frec.reserve(rec.size() * sizeof(FastRec)));
  RF_HIP(hipMemcpy(p->frec.get(), rec.data(), rec.size() * sizeof(FastRec), hipMemcpyHostToDevice));
  p->fnbins = (int)rec.size();
  // side buffer of the repaired kz = 0 slots (one complex per mode (ix, iy): 8 MB at 1024^2 float32), filled and read inside the
  // generation pass by the rank that owns kz = 0 -- every rank in replicated-generation mode
  RF_HIP(p->fixbuf.reserve((size_t)p->nx * p->ny * p->csize));
  p->have_fast = true;
  return 0;
}

// bytes of a sub-slab of the exchange in the field buffer (one sub-slab: the whole kz slab)
size_t chunk_bytes(const rf_plan* p) { return p->w_bytes / (size_t)route(p).chunks; }

// x pass (generation or API k-space fused into its load) into buffer W on stream sx
// Replicated-generation mode of a multi-rank plan (RF_FLAG_REPLICATED_GENERATION): the native generator is keyed by
// the global cell index and the x pass reads nothing, so a rank can generate ALL of k space on the fly, run the
// full x-FFT and store only its own x slab [rank*nxl, (rank+1)*nxl); the y and z passes are then local and no
// all-to-all is needed (only the 2-double all-reduce of the moments).  It trades P-fold redundant x-pass arithmetic
// for the exchange: a win when the exchange is slower than (P-1) x passes -- 2 GPUs share ONE xGMI link.

// (kz0c, nzlc >= 0: a sub-slab of this rank's planes instead of all of them -- W then points at the sub-slab's own region)
// (tl: the fast generation's kz = 0 tiles are rf_kernel_ms's entry 4; the caller marks the end of the pass)
int queue_x(rf_plan* p, const CallDesc& cd, const GenParams& gp, const void* kspace, void* W, hipStream_t sx, Timeline* tl, int kz0c, int nzlc) {
  // which kernel, on which deviates, and whether it serves the call's stored / emitted potential: rf_source.h (resident deviates take
  // the fast float32 sigma path too; host-supplied ones, the parity mode, keep the exact reference dtype chain)
  const Source src = source(p, cd.ask(kspace != nullptr));
  RF_REQUIRE(!src.refused(), src.refusal);
  const bool rep = route(p).replicates(), fast = src.fast();
  const long long nzl = nzlc >= 0 ? nzlc : (rep ? p->nzc : p->nzl);     // kz planes generated by this call (nz/2 on one GPU)
  const int kz0 = kz0c >= 0 ? kz0c : (rep ? 0 : p->kz0);
  // W == p->X: the blocked intermediate [x block][kz tile][ny][rb][TC] -- a tile (all nx rows of TC adjacent kz of one iy) is
  // nx / rb contiguous chunks of rb * TC cells there
  const ColGeom gx = (W == p->X.ptr && W != nullptr)
                         ? xblock_x_geom(p->nx, p->ny, nzl, col_gen_tile_cols(p->f64, p->nx), xpose_row_block(p))
                         : ColGeom{(long long)p->ny * nzl, 0, (long long)p->ny * nzl};
  hipEvent_t after_repair = nullptr;
  if (fast) RF_HIP(mark(tl, rft::EXTRA, sx, &after_repair));       // in front of the pass; recorded again by the launcher if it splits
  FastGenParams fgp = make_fast(p, cd, gp.seed, gp.seed_dev != nullptr, gp.seed_dev);
  if (src.reads_pairs32()) {
    fgp.noise32 = reinterpret_cast<const cplx<float>*>(p->mt.scratch.ptr);      // (a later float64 replay reuses the scratch: the float32 claim goes with it)
    fgp.rowtab = reinterpret_cast<const RowLoc*>(p->mt.rowtab.ptr); fgp.seg_cap = p->mt.seg_cap;
  }
  else if (src.kind == Source::FastDeviates64) fgp.noise = gp.noise;
  if (fast)
    RF_HIP(launch_col_fastgen(p->f64, p->nx, W, gx, (long long)p->ny * nzl, fgp,
                              kz0, (int)nzl, p->tw_x.ptr, sx, after_repair,
                              rep ? p->rank * p->nxl : 0, rep ? (p->rank + 1) * p->nxl : 1 << 30, cd.pot_target, p->fixbuf.ptr));
  else
    RF_HIP(launch_col_gen(p->f64, p->nx, W, gx, (long long)p->ny * nzl, gp, kspace, kz0, (int)nzl, p->tw_x.ptr, sx));
  return 0;
}

// The device table of destination bases the storing y pass reads (rf_fft.h DirectColIO): for receive buffer b, sub-slab c and
// destination rank h, cell `off` of block h of the local sub-slab lands at  R_h + (rank * C + c) * blk_c + off  =  tab + h * blk_c + off.
int rebuild_peer_tab(rf_plan* p) {
  const int C = route(p).chunks, P = p->nranks;
  RF_REQUIRE((int)p->peer_R[0].size() == P && (int)p->peer_R[1].size() == P, "direct exchange: the peers' receive buffers are not known");
  RF_REQUIRE(col_direct_supported(p->f64, p->ny, p->nzl / C),
             "direct exchange: a y-pass tile would straddle two x planes (nz / (2 ranks chunks) is narrower than the tile)");
  const long long blk_c = (long long)p->nxl * p->ny * (p->nzl / C) * (long long)p->csize;
  std::vector<void*> h_tab((size_t)2 * C * P);
  for (int b = 0; b < 2; ++b)
    for (int c = 0; c < C; ++c)
      for (int h = 0; h < P; ++h)
        h_tab[((size_t)b * C + c) * P + h] = p->peer_R[b][h] ? (char*)p->peer_R[b][h] + ((long long)p->rank * C + c - h) * blk_c : nullptr;
  RF_HIP(hipStreamSynchronize(p->stream));
  if (p->comm_stream) RF_HIP(hipStreamSynchronize(p->comm_stream));
  p->peer_tab_chunks = 0;
  RF_HIP(p->peer_tab.release());
  RF_HIP(p->peer_tab.reserve(h_tab.size() * sizeof(void*)));
  RF_HIP(hipMemcpy(p->peer_tab.get(), h_tab.data(), h_tab.size() * sizeof(void*), hipMemcpyHostToDevice));
  p->peer_tab_chunks = C;
  return 0;
}

// the barrier between the peers' stores into a receive buffer and its readers (and, the other way, between the readers of a receive
// buffer and the next stores into it): a 2-double all-reduce on its own scratch words.  Virtual ranks (no communicator) are ordered
// by the host that drives them.
int direct_barrier(rf_plan* p, hipStream_t s) {
  if (p->nranks > 1 && p->comm) RF_NCCL(g_rccl.AllReduce(p->coll_scratch.get() + 2, p->coll_scratch.get() + 2, 2, ncclFloat64, ncclSum, p->comm, s));
  return 0;
}

// the y pass of sub-slab c (the whole kz slab when the plan does not chunk) out of W into the peers' receive buffers number `rbuf`
int queue_y_direct(rf_plan* p, const void* W, int rbuf, hipStream_t s, int c) {
  const int C = route(p).chunks;
  RF_REQUIRE(p->peer_tab.get() && p->peer_tab_chunks == C && c >= 0 && c < C, "direct exchange: the destination table does not match the plan's exchange chunks");
  RF_REQUIRE(p->peer_R[rbuf][p->rank] != nullptr, "direct exchange: the second receive buffer does not exist");
  const long long nzc_ = p->nzl / C;
  const ColGeom gy{nzc_, (long long)p->ny * nzc_, nzc_};
  int shift = 0;
  while ((1 << shift) < p->nxl) ++shift;
  RF_HIP(launch_col_direct(p->f64, p->ny, (const char*)W + (size_t)c * chunk_bytes(p), gy, p->peer_tab.get() + ((size_t)rbuf * C + c) * p->nranks, shift,
                           (long long)p->nx * nzc_, p->tw_y.ptr, s));
  return 0;
}

int queue_exchange_rccl(rf_plan* p, const void* W, void* R, hipStream_t s, int chunk = -1, bool plain = false);

// The forward half of a plan that exchanges, sub-slab by sub-slab (one sub-slab: the whole kz slab), W -> receive buffers.  Per sub-slab c:
// the x pass on A into region c of W, then either the storing y pass on E into the peers' receive buffers number `rbuf` (r.direct), or the
// plain y pass in place on A and, where the caller hands over the receive buffer R, the sub-slab's grouped send / receive on E.
// E != A: what goes to E follows the x / y pass of its sub-slab behind chunk_ev[c] and runs beside the x pass of sub-slab c + 1 (the stores
// and the sends are link-bound on a real job); the caller has put E behind whatever frees the receive buffers.
// tl: one sub-slab marks the x entry behind the x pass and the y entry behind the y pass; in sub-slabs the whole forward half is the x
// entry (E != A: E is still busy -- the x passes' end stands for both).
int queue_forward(rf_plan* p, const Route& r, const CallDesc& cd, const GenParams& gp, const void* kspace, void* W, int rbuf, void* R,
                  hipStream_t A, hipStream_t E, Timeline* tl) {
  const int C = r.chunks, nzc_ = p->nzl / C;
  const ColGeom gy{nzc_, (long long)p->ny * nzc_, nzc_};
  if (E != A) RF_HIP(p->chunk_ev.ensure(C + 1, hipEventDisableTiming));
  for (int c = 0; c < C; ++c) {
    char* Wc = (char*)W + (size_t)c * chunk_bytes(p);
    if (C == 1) { if (int rc = queue_x(p, cd, gp, kspace, W, A, tl)) return rc; }
    else if (int rc = queue_x(p, cd, gp, kspace, Wc, A, nullptr, p->kz0 + c * nzc_, nzc_)) return rc;
    if (C == 1) RF_HIP(mark(tl, rft::X, A));
    if (r.direct) {
      if (E != A) RF_HIP(hop(p->chunk_ev[c], A, E));
      if (int rc = queue_y_direct(p, W, rbuf, E, c)) return rc;
    } else {
      RF_HIP(launch_col_plain(p->f64, p->ny, +1, Wc, gy, (long long)p->nx * nzc_, p->tw_y.ptr, A));
    }
    if (C == 1) RF_HIP(mark(tl, rft::Y, A));
    if (!r.direct && R) {
      if (E != A) RF_HIP(hop(p->chunk_ev[c], A, E));
      if (int rc = queue_exchange_rccl(p, W, R, E, c)) return rc;
    }
  }
  if (C > 1) RF_HIP(mark(tl, rft::X, A));
  return 0;
}

// x pass (generation or API k-space fused into its load) + y pass of buffer W on stream s, with a mark behind either: the forward half
// without its exchange (the step-wise rf_slab_forward*, the batches).  A plan in direct mode stores into the peers' receive buffers
// `rbuf`, and what follows is the z pass, not an exchange.
int queue_xy(rf_plan* p, const CallDesc& cd, const GenParams& gp, const void* kspace, void* W, hipStream_t s, Timeline* tl, int rbuf) {
  const Route r = route(p);
  if (r.exchanges()) return queue_forward(p, r, cd, gp, kspace, W, rbuf, nullptr, s, s, tl);
  const bool rep = r.replicates();
  const long long nzl = rep ? p->nzc : p->nzl, nxp = rep ? p->nxl : p->nx;      // the local array is [nxp][ny][nzl]
  const ColGeom gy{nzl, (long long)p->ny * nzl, nzl};
  if (int rc = queue_x(p, cd, gp, kspace, W, s, tl)) return rc;
  RF_HIP(mark(tl, rft::X, s));
  RF_HIP(launch_col_plain(p->f64, p->ny, +1, W, gy, nxp * nzl, p->tw_y.ptr, s));
  RF_HIP(mark(tl, rft::Y, s));
  return 0;
}

// multi-rank: z pass on the local x slab, rows gathered from the P received blocks in R; output
// (dense real [nxl][ny][nz]) into W, then the local (sum, sumsq)
int queue_z_slab(rf_plan* p, const void* R, void* W, double* stats_out, hipStream_t s) {
  const long long nrows = (long long)p->nxl * p->ny;
  const long long nzseg = p->nzl / route(p).chunks;            // planes per received segment: nranks * chunks of them make a row
  RF_HIP(launch_row_c2r_gather(p->f64, p->nzc, R, W, nrows, inv_cells(p), (int)nzseg, nrows * nzseg, p->tw_z.ptr, p->partials.get(), s));
  RF_HIP(launch_reduce_partials(p->partials.get(), p->npartials, stats_out, p->partials.get() + 2 * p->npartials, s));
  p->has.field_gathered(W);
  return 0;
}

// replicated generation, behind queue_xy: the local array already is this rank's x slab [nxl][ny][nz/2] -- the z pass on it and its
// (sum, sumsq) into pair `slot` (the z entry of a timed call), then, allreduce > 0, the global sums of the first so many pairs
int replicated_z(rf_plan* p, int slot, int allreduce, Timeline* tl) {
  RF_HIP(launch_row_c2r(p->f64, (int)p->nzc, p->W.ptr, (long long)p->nxl * p->ny, inv_cells(p), p->tw_z.ptr, p->partials.get(), p->stream));
  RF_HIP(launch_reduce_partials(p->partials.get(), p->npartials, p->stats.get() + 2 * slot, p->partials.get() + 2 * p->npartials, p->stream));
  RF_HIP(mark(tl, rft::Z, p->stream));
  if (allreduce > 0 && p->comm) RF_NCCL(g_rccl.AllReduce(p->stats.get(), p->stats.get(), 2 * (size_t)allreduce, ncclFloat64, ncclSum, p->comm, p->stream));
  return 0;
}

// multi-rank: the single all-to-all between the y and z passes.  Rank g sends to rank h the block
// [x in slab h][all y][kz in slab g], which is contiguous in W because x is the slowest axis.
// (chunk >= 0: sub-slab `chunk` only -- RF_FLAG_EXCHANGE_CHUNKS; -1: everything, all chunks of a chunked plan in ONE group;
// plain = true: the unchunked block layout whatever the flag says, as the forward transform's reverse exchange uses it)
int queue_exchange_rccl(rf_plan* p, const void* W, void* R, hipStream_t s, int chunk, bool plain) {
  RF_REQUIRE(p->nranks == 1 || p->comm != nullptr || p->standin_wg > 0, "rf_comm_init has not been called on this multi-rank plan");
  const int C = plain ? 1 : route(p).chunks;
  const size_t blk = (size_t)p->nxl * p->ny * p->nzl * p->csize / (size_t)C, cb = p->w_bytes / (size_t)C;
  const int c0 = chunk >= 0 ? chunk : 0, c1 = chunk >= 0 ? chunk + 1 : C;
  // block h of sub-slab c of W -> segment (this rank, c) of rank h's R
  auto src = [&](int c, int h) { return (const char*)W + (size_t)c * cb + (size_t)h * blk; };
  auto dst = [&](int c, int g) { return (char*)R + ((size_t)g * C + c) * blk; };
  for (int c = c0; c < c1; ++c)
    RF_HIP(hipMemcpyAsync(dst(c, p->rank), src(c, p->rank), blk, hipMemcpyDeviceToDevice, s));
  if (p->nranks == 1) return 0;        // forced slab path of a single-rank plan: the own block is everything
  if (!p->comm) {
    // exchange stand-in of a virtual rank (diagnostics): what this rank's RCCL kernels would do to ITS memory and compute units --
    // read the nranks - 1 blocks it sends, write the nranks - 1 segments it receives -- by a copy kernel of fixed width; the
    // segments hold this rank's own data for other x slabs (not a field: the timing of the overlapped passes is the point)
    RF_REQUIRE(p->nranks <= 17, "the exchange stand-in serves up to 17 ranks");
    for (int c = c0; c < c1; ++c) {
      const void* sp[16]; void* dp[16];
      int nb = 0;
      for (int h = 0; h < p->nranks; ++h) if (h != p->rank) { sp[nb] = src(c, h); dp[nb] = dst(c, h); ++nb; }
      RF_HIP(launch_exchange_standin(sp, dp, nb, blk, p->standin_wg, p->standin_read_pct, p->standin_write_pct, (unsigned*)p->coll_scratch.get(), s));
    }
    return 0;
  }
  // (a failing send / receive must not leave the group open on this communicator: the first error is kept, the group is always closed)
  RF_NCCL(g_rccl.GroupStart());
  ncclResult_t first = ncclSuccess;
  const char* what = "";
  for (int c = c0; c < c1 && first == ncclSuccess; ++c)
    for (int h = 0; h < p->nranks && first == ncclSuccess; ++h) {
      if (h == p->rank) continue;
      if ((first = g_rccl.Send(src(c, h), blk, ncclUint8, h, p->comm, s)) != ncclSuccess) { what = "ncclSend"; break; }
      if ((first = g_rccl.Recv(dst(c, h), blk, ncclUint8, h, p->comm, s)) != ncclSuccess) { what = "ncclRecv"; break; }
    }
  const ncclResult_t end = g_rccl.GroupEnd();
  if (first != ncclSuccess) return fail(5, std::string(what) + " inside the grouped exchange failed: " + g_rccl.GetErrorString(first));
  RF_NCCL(end);
  return 0;
}

// second (send, receive) buffer pair, exchange stream and events of the pipelined batches (each step idempotent: whatever failed is
// tried again by the next call)
int ensure_batch_buffers(rf_plan* p) {
  RF_HIP(p->W2.reserve(p->w_bytes));
  RF_HIP(p->R2.reserve(p->w_bytes));
  RF_HIP(p->comm_stream.create(hipStreamNonBlocking));
  RF_HIP(p->pev.ensure(6, hipEventDisableTiming));
  return 0;
}

// What both pipelined batches end with, the last z pass being queued on A: the moments of all n realisations in ONE all-reduce on S, the
// stream that drives the communicator inside the batch (S != A: behind the last z pass's event, and A waits for it through `back`); the
// call's end; the last field in the buffer of its turn -- or none, after a stand-in (this rank's own data lies in the segments)
int batch_tail(rf_plan* p, int n, hipStream_t A, hipStream_t S, hipEvent_t z_done, hipEvent_t back, void* last, bool standin) {
  if (p->nranks > 1 && p->comm) {        // (no communicator: a virtual rank under a stand-in, local moments only)
    if (S != A) RF_HIP(hipStreamWaitEvent(S, z_done, 0));
    RF_NCCL(g_rccl.AllReduce(p->stats.get(), p->stats.get(), 2 * (size_t)n, ncclFloat64, ncclSum, p->comm, S));
    if (S != A) RF_HIP(hop(back, S, A));
  }
  RF_HIP(p->tl.end(A));
  p->has.field_ready(last, n - 1);
  if (standin) p->has.not_a_field();
  return 0;
}

// Pipelined batch of a plan in direct mode.  The y pass of realisation i stores into the PEERS' receive buffers i % 2 -- it is the
// exchange, and on a real job it runs at the speed of the links -- so it goes to the exchange stream Y, where it runs beside the z pass of
// realisation i - 1 and the x pass of realisation i + 1 on the compute stream A; B(i), a tiny all-reduce on Y, tells every rank that
// all y(i) and all z(i - 1) are done:
//   A:  x(0) | x(1)          z(0) | x(2)          z(1) | ...
//   Y:  B(-1) y(0) B(0)    | y(1)   B(1)        | y(2)   B(2)        | ...
// y(i) waits for x(i) (event) and follows B(i - 1) on Y: no peer still reads its receive buffer i % 2 (z(i - 2) is inside B(i - 1));
// z(i) waits for B(i): every peer's stores of realisation i have landed; x(i + 2), which overwrites the send buffer y(i) read, follows
// z(i) on A.  The local HBM traffic is that of the passes alone: no send-side reads, no receive-side writes by copy kernels.
// (direct_overlap = 0: everything on A in the order x(i) y(i) z(i - 1) B(i).)
int slab_batch_direct(rf_plan* p, const Route& r, const uint64_t* seeds, int n) {
  RF_REQUIRE(p->nranks == 1 || p->comm || p->direct_standin, "virtual ranks linked for the direct exchange run step by step (rf_slab_forward, rf_slab_backward)");
  void* Wb[2] = {p->W.ptr, p->W2.ptr};
  void* Rb[2] = {p->R.ptr, p->R2.ptr};
  const hipEvent_t *ev_bar = p->pev.ev.data() + 2, *ev_z = ev_bar + 2;
  const bool two = p->direct_overlap != 0;
  hipStream_t A = p->stream, Y = two ? p->comm_stream : p->stream;
  RF_HIP(p->tl.begin(A, false));
  if (two) RF_HIP(hop(ev_z[1], A, Y));                            // whatever the plan's stream did before
  if (int rc = direct_barrier(p, Y)) return rc;                   // B(-1): nobody is still reading (or sending from) a receive buffer
  for (int i = 0; i <= n; ++i) {
    const int b = i & 1, pb = (i - 1) & 1;
    if (i < n) {
      // (sub-slab by sub-slab when the plan chunks: x(c) on A, the stores of sub-slab c on Y behind an event)
      if (int rc = queue_forward(p, r, CallDesc(), make_gen(p, seeds[i], RF_NOISE_NATIVE), nullptr, Wb[b], b, nullptr, A, Y, nullptr)) return rc;
    }
    if (i >= 1) {
      if (two) RF_HIP(hipStreamWaitEvent(A, ev_bar[pb], 0));
      if (int rc = queue_z_slab(p, Rb[pb], Wb[pb], p->stats.get() + 2 * (i - 1), A)) return rc;
      if (two) RF_HIP(hipEventRecord(ev_z[pb], A));
    }
    if (i < n) {
      if (two && i >= 1) RF_HIP(hipStreamWaitEvent(Y, ev_z[pb], 0));
      if (int rc = direct_barrier(p, Y)) return rc;               // B(i)
      if (two) RF_HIP(hipEventRecord(ev_bar[b], Y));
    }
  }
  const int lb = (n - 1) & 1;
  return batch_tail(p, n, A, Y, ev_z[lb], ev_bar[lb], Wb[lb], p->direct_standin);
}

// room for the (sum, sumsq) pairs of n realisations (captured batch graphs carry the array's address: they go)
int ensure_stats(rf_plan* p, int n) {
  if (p->stats.bytes >= 2 * (size_t)n * sizeof(double)) return 0;
  RF_HIP(hipStreamSynchronize(p->stream));
  drop_graphs(p);
  RF_HIP(p->stats.reserve(2 * (size_t)(n + 64) * sizeof(double)));
  return 0;
}

// Pipelined batch on the slab path: realisation i+1's generation + x + y passes (compute stream) run
// while realisation i's all-to-all is in flight (exchange stream); two (send, receive) buffer pairs.
//   compute: x,y(0) | x,y(1)   z(0) | x,y(2)   z(1) | ...            (in order on p->stream)
//   exchange:        | exch(0)       | exch(1)       | ...            (in order on p->comm_stream)
// z(i) waits for exch(i); exch(i) waits for x,y(i) and -- because it overwrites R[i%2] -- for z(i-2).
// One all-reduce of all n (sum, sumsq) pairs at the end, on the exchange stream too: ONE communicator is only ever driven from ONE
// stream inside a batch.
int slab_batch(rf_plan* p, const Route& r, const uint64_t* seeds, int n) {
  if (int rc = ensure_stats(p, n)) return rc;
  if (r.replicates()) {          // no exchange to overlap: realisations back to back, one all-reduce at the end
    RF_HIP(p->tl.begin(p->stream, false));
    for (int i = 0; i < n; ++i) {
      if (int rc = queue_xy(p, CallDesc(), make_gen(p, seeds[i], RF_NOISE_NATIVE), nullptr, p->W.ptr, p->stream, nullptr)) return rc;
      if (int rc = replicated_z(p, i, i + 1 == n ? n : 0, nullptr)) return rc;
    }
    RF_HIP(p->tl.end(p->stream));
    p->has.field_ready(p->W.ptr, n - 1);
    return 0;
  }
  if (int rc = ensure_batch_buffers(p)) return rc;
  if (r.direct) return slab_batch_direct(p, r, seeds, n);
  void* Wb[2] = {p->W.ptr, p->W2.ptr};
  void* Rb[2] = {p->R.ptr, p->R2.ptr};
  const hipEvent_t *ev_fwd = p->pev.ev.data(), *ev_exch = ev_fwd + 2, *ev_z = ev_fwd + 4;
  hipStream_t A = p->stream, C = p->comm_stream;
  RF_HIP(p->tl.begin(A, false));
  for (int i = 0; i <= n; ++i) {
    if (i < n) {
      const int b = i & 1;
      if (int rc = queue_forward(p, r, CallDesc(), make_gen(p, seeds[i], RF_NOISE_NATIVE), nullptr, Wb[b], 0, nullptr, A, A, nullptr)) return rc;
      RF_HIP(hop(ev_fwd[b], A, C));
      if (i >= 2) RF_HIP(hipStreamWaitEvent(C, ev_z[b], 0));          // R[b] still being read by z(i-2)?
      if (int rc = queue_exchange_rccl(p, Wb[b], Rb[b], C)) return rc;
      RF_HIP(hipEventRecord(ev_exch[b], C));
    }
    if (i >= 1) {
      const int pb = (i - 1) & 1;
      RF_HIP(hipStreamWaitEvent(A, ev_exch[pb], 0));
      if (int rc = queue_z_slab(p, Rb[pb], Wb[pb], p->stats.get() + 2 * (i - 1), A)) return rc;
      RF_HIP(hipEventRecord(ev_z[pb], A));
    }
  }
  const int lb = (n - 1) & 1;
  return batch_tail(p, n, A, C, ev_z[lb], ev_exch[lb], Wb[lb], p->nranks > 1 && !p->comm);
}

// x planes per slab of the y / z passes of a single-rank plan (0: whole-grid passes).  The y pass of a slab leaves it in the
// 256 MiB Infinity Cache for the z pass that follows at once; slabs much smaller than the cache make the launches too small
// (1024^3 float32, MI355X, 20 realisations per graph: 4.74 ms whole grid, 4.53-4.57 ms with 64-plane = 256 MiB slabs, 4.66 with 56,
// 4.70 with 72 ... 128, 4.74 with 48, 5.6 ms with 16; 2048^3: 44.5 -> 43.7-43.9 ms; 512^3: 0.545 -> 0.537 ms).
int yz_slab_planes(const rf_plan* p) {
  if (!route(p).single() || p->yz_slab == 0) return 0;
  const long long plane = (long long)p->ny * p->nzl * (long long)p->csize;
  long long B = p->yz_slab;
  if (B < 0) {
    if (p->f64 && !p->sink_host) return 0;      // float64 passes: within 1 % of the whole-grid launches at every slab size measured (9.32-9.53 against 9.41 ms); slabs anyway when a host sink wants them one by one
    const long long target = 256LL << 20;              // the Infinity Cache (RF_FLAG_YZ_SLAB_PLANES sets another slab size per plan)
    B = 1;
    while (2 * B * plane <= target) B *= 2;
  }
  if (B >= p->nx) return 0;
  // whole z-pass workgroups per slab (the last slab may be smaller), at the offsets the whole-grid launch would give them
  const long long tiles1 = row_c2r_tiles(p->f64, (int)p->nzc, p->ny);
  if (tiles1 <= 0 || tiles1 * p->nx != p->npartials) return 0;
  return (int)B;
}

// y and z passes of a single-rank plan + the moments into stats_out[0..1], slab by slab when yz_slab_planes() says so.  The x
// pass has left its output either in W (plain layout: both passes in place) or in the blocked intermediate X (y pass in place
// on X, z pass gathering X -> W).
// Host sink (rf_set_host_sink).  The z pass of a slab of x planes has been queued on s: mark that point with an event ...
int sink_mark(rf_plan* p, int slab, hipStream_t s) {
  RF_HIP(p->sink_ev.ensure(slab + 1, hipEventDisableTiming));
  RF_HIP(hipEventRecord(p->sink_ev[slab], s));
  return 0;
}
// ... and, once the launches of the NEXT slab are queued too (the GPU has work while the host waits here), copy planes [x0, x0 + nb)
// to the armed host buffer: an ordinary device -> host copy into pageable memory on dl_stream behind the slab's event -- it returns
// when the rows are in the caller's memory.  (The host buffer is deliberately NOT registered with hipHostRegister: round 6 first
// built it that way, and later device -> host copies of the same process then aborted now and then inside the runtime.)
int sink_copy(rf_plan* p, const void* W, long long x0, long long nb, int slab) {
  RF_HIP(hipStreamWaitEvent(p->dl_stream, p->sink_ev[slab], 0));
  const size_t rsize = p->csize / 2, width = (size_t)p->nz * rsize;
  const size_t hpitch = p->sink_layout == RF_LAYOUT_PADDED ? (size_t)(p->nz + 2) * rsize : width;
  RF_HIP(hipMemcpy2DAsync((char*)p->sink_host + (size_t)x0 * p->ny * hpitch, hpitch, (const char*)W + (size_t)x0 * p->ny * width, width, width,
                          (size_t)nb * p->ny, hipMemcpyDeviceToHost, p->dl_stream));
  RF_HIP(hipStreamSynchronize(p->dl_stream));
  return 0;
}
// ... after the last slab: the armed call returns with the field on the host (one shot)
int sink_finish(rf_plan* p) {
  p->sink_host = nullptr;
  p->sink_delivered = true;
  return 0;
}

// tl: a mark behind every launch (rf_kernel_ms: [1], [2] = the sums over the slabs' y and z launches; a merged launch counts as y) and,
// the call's last pass being queued here, its end -- in front of the last slab's copy to a host sink, which waits on the host.
int queue_yz(rf_plan* p, const CallDesc& cd, void* W, hipStream_t s, double* stats_out, Timeline* tl) {
  const long long nzl = p->nzl;
  const bool sink = p->sink_host != nullptr && !cd.zscale && !cd.intermediate && !capturing(s);      // (a captured batch keeps its fields on the device)
  const double scale = inv_cells(p);
  const bool xp = p->X.ptr && xpose_ok(p);
  const long long rb = xpose_row_block(p), tc = col_tile_cols(p->f64, p->ny);
  const ColGeom gy = xp ? xblock_y_geom(p->nx, p->ny, nzl, tc, rb) : ColGeom{nzl, (long long)p->ny * nzl, nzl};
  const YzSlabs sl = yz_slabs(p->nx, yz_slab_planes(p), xp, (int)rb);
  const long long B = sl.planes, plane = (long long)p->ny * nzl * (long long)p->csize, tiles_per_plane = p->npartials / p->nx;
  // untimed single-rank float32 realisations at the sizes rf_k_yz.hip serves: the z pass of slab i and the y pass of slab i + 1 share a
  // launch (the next slab's y tiles fill the CUs the draining z pass leaves idle); timed calls keep one launch per pass and slab, so
  // that rf_kernel_ms still means what it says
  // (rf_set_merged_yz(2) merges timed calls too, with a mark behind every launch: rf_merged_yz_ms)
  // (the last slab may be smaller -- a slab size that does not divide nx: RF_FLAG_YZ_SLAB_PLANES -- as long as both sizes fit the kernel)
  const bool merge = p->yz_merge >= ((tl && tl->detailed) ? 2 : 1) && !xp && !cd.zscale && sl.count > 1 &&
                     yz_merged_fits(p->f64, p->ny, (int)p->nzc, gy, B * p->ny, B * nzl) &&
                     (sl.last == B || yz_merged_fits(p->f64, p->ny, (int)p->nzc, gy, B * p->ny, sl.last * nzl));
  auto planes_of = [&](int i) { return i + 1 < sl.count ? B : (long long)sl.last; };
  for (int i = 0; i < sl.count; ++i) {
    const long long x0 = (long long)i * B, nb = planes_of(i);      // planes [x0, x0 + nb)
    char* Ws = (char*)W + x0 * plane;
    char* Xs = xp ? (char*)p->X.ptr + x0 * plane : nullptr;        // (x blocks are contiguous and as large as their planes)
    double* part = p->partials.get() + 2 * x0 * tiles_per_plane;
    if (!merge || i == 0) {                                        // (merged: the launch of slab i - 1 has run this slab's y pass)
      if (xp) RF_HIP(launch_col_xpose(p->f64, p->ny, Xs, gy, Xs, gy, nb * nzl, p->tw_y.ptr, s));
      else RF_HIP(launch_col_plain(p->f64, p->ny, +1, Ws, gy, nb * nzl, p->tw_y.ptr, s));
      RF_HIP(mark(tl, rft::Y, s));
    }
    const bool with_next = merge && i + 1 < sl.count;              // this slab's z pass and the next slab's y pass in one launch
    if (with_next) RF_HIP(launch_yz_merged(p->f64, p->ny, (int)p->nzc, Ws, nb * p->ny, scale, p->tw_z.ptr, part, Ws + B * plane, gy, planes_of(i + 1) * nzl, p->tw_y.ptr, s));
    else if (xp) RF_HIP(launch_row_c2r_xgather(p->f64, (int)p->nzc, Xs, Ws, nb * p->ny, scale, (int)tc, (int)rb, p->ny, p->tw_z.ptr, part, s));
    else if (cd.zscale) RF_HIP(launch_row_c2r_zscale(p->f64, (int)p->nzc, Ws, nb * p->ny, scale, cd.zscale, p->tw_z.ptr, part, s));
    else RF_HIP(launch_row_c2r(p->f64, (int)p->nzc, Ws, nb * p->ny, scale, p->tw_z.ptr, part, s));
    RF_HIP(mark(tl, with_next ? rft::Y : rft::Z, s, nullptr, with_next));
    if (sink) {
      if (int rc = sink_mark(p, i, s)) return rc;
      if (i > 0) if (int rc = sink_copy(p, W, x0 - B, B, i - 1)) return rc;                          // (slab i - 1, while the GPU runs slab i)
    }
  }
  if (!cd.intermediate) RF_HIP(launch_reduce_partials(p->partials.get(), p->npartials, stats_out, p->partials.get() + 2 * p->npartials, s));
  if (tl) RF_HIP(tl->end(s));
  if (sink) {
    if (int rc = sink_copy(p, W, (long long)(sl.count - 1) * B, sl.last, sl.count - 1)) return rc;
    return sink_finish(p);
  }
  return 0;
}

// the whole single-rank pipeline: x pass (generation or API k-space fused into its load; into the transposed intermediate
// when the plan uses it), then queue_yz
int queue_xyz(rf_plan* p, const CallDesc& cd, const GenParams& gp, const void* kspace, void* W, hipStream_t s, double* stats_out, Timeline* tl) {
  if (!capturing(s))                               // (no allocation inside a graph capture: batch_prepare() has done it)
    if (int rc = ensure_x(p)) return rc;
  const bool xp = p->X.ptr && xpose_ok(p);
  if (int rc = queue_x(p, cd, gp, kspace, xp ? p->X.ptr : W, s, tl)) return rc;
  RF_HIP(mark(tl, rft::X, s));
  return queue_yz(p, cd, W, s, stats_out, tl);
}

// the launches behind the sequences of rf_generic.h (generic_c2r_seq / generic_r2c_seq / generic_c2c_seq) on the plan's stream
struct HipGenericOps {
  rf_plan* p;
  hipStream_t s;
  // per-kernel times of a realisation (rf_kernel_ms): the inverse sequence launches on the x, y and z root tables in that order; when
  // the phase changes, what was queued until now belongs to the part that just ended
  Timeline* tl = nullptr;
  int phase = 0;
  int enter(int ph) {
    if (ph > phase) { RF_HIP(mark(tl, Part(phase), s)); phase = ph; }
    return 0;
  }
  const void* root(int which) const { return which == 0 ? p->tw_x.ptr : (which == 1 ? p->tw_y.ptr : p->tw_z.ptr); }
  int axis(const void* src, void* dst, const GenericAxis& ax, long long stride, long long inner, long long outer, long long nlines, int which, int sign, double scale) {
    if (int rc = enter(which)) return rc;
    RF_HIP(launch_generic_axis(p->f64, src, dst, ax, stride, inner, outer, nlines, root(which), sign, scale, s));
    return 0;
  }
  // the x pass from a descriptor (rf_generic.h generic_c2r_from_seq): the generator (GenParams; no array), or one component of the
  // gradient / Hessian of the array S (GradParams / HessParams) with its factor applied to the cells the pass loads
  int axis_from(const GenParams& gp, const void*, void* dst, const GenericAxis& ax, long long stride, long long inner, long long outer, long long nlines, int which, int sign, double scale) {
    RF_HIP(launch_generic_axis_gen(p->f64, gp, dst, ax, stride, inner, outer, nlines, root(which), sign, scale, s));
    return 0;
  }
  template <class P>
  int axis_from(const P& dp, const void* S, void* dst, const GenericAxis& ax, long long stride, long long inner, long long outer, long long nlines, int which, int sign, double scale) {
    RF_HIP(launch_generic_axis_deriv(p->f64, dp, S, dst, ax, stride, inner, outer, nlines, root(which), sign, scale, s));
    return 0;
  }
  // ... and, for a plan whose x axis is split, the same cells by a launch of its own into a scratch array (rf_kernel_ms: entry 4)
  int materialise(const GenParams& gp, const void*, void* K) {
    RF_HIP(launch_gen_kspace(p->f64, K, gp, s));
    RF_HIP(mark(tl, rft::EXTRA, s));
    return 0;
  }
  template <class P>
  int materialise(const P& dp, const void* S, void* K) {
    RF_HIP(launch_derivative(p->f64, S, K, dp, s));
    RF_HIP(mark(tl, rft::EXTRA, s));
    return 0;
  }
  int lines(const void* src, void* dst, const GenericLines& L, int which) {
    if (int rc = enter(which)) return rc;
    RF_HIP(launch_generic_lines(p->f64, src, dst, L, root(which), s));
    return 0;
  }
  int row_c2r(const void* G, void* W, double scale) {
    if (int rc = enter(2)) return rc;
    RF_HIP(launch_generic_row_c2r(p->f64, G, W, p->gdims.az, (long long)p->nx * p->ny, p->tw_z.ptr, scale, p->partials.get(), s));
    return 0;
  }
  int row_r2c(const void* W, void* G) {
    RF_HIP(launch_generic_row_r2c(p->f64, W, G, p->gdims.az, (long long)p->nx * p->ny, p->tw_z.ptr, s));
    return 0;
  }
  int untangle(const void* G, void* Z) { if (int rc = enter(2)) return rc; RF_HIP(launch_generic_untangle(p->f64, G, Z, (int)p->nzc, (long long)p->nx * p->ny, p->tw_z.ptr, s)); return 0; }
  int tangle(const void* Z, void* G) { RF_HIP(launch_generic_tangle(p->f64, Z, G, (int)p->nzc, (long long)p->nx * p->ny, p->tw_z.ptr, s)); return 0; }
  int moments(const void* W) { RF_HIP(launch_generic_moments(p->f64, W, (long long)p->nx * p->ny * p->nz, p->partials.get(), p->npartials, s)); return 0; }
  int copy(void* dst, const void* src, size_t bytes) { RF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s)); return 0; }
};
bool generic_any_long(const rf_plan* p) { return p->gdims.lx.split() || p->gdims.ly.split() || p->gdims.lz.split(); }
// the second scratch array, for plans with an axis in the four-step form
int ensure_g2(rf_plan* p) {
  if (generic_any_long(p)) RF_HIP(p->G2.reserve(p->unpacked ? p->w_bytes : p->k_bytes));
  return 0;
}

// non-power-of-two grid: API-layout half spectrum K -> x pass into G -> y pass -> contiguous c2r pass into W (rf_generic.h
// generic_c2r_seq: axes too long for one line of the LDS take the four-step form through the scratch arrays), (sum, sumsq) into stats_out.
// from != null: the x pass takes its cells from that descriptor instead of loading K (generic_c2r_from_seq) -- GenParams: it generates
// the half spectrum (RF_FLAG_FUSED_GENERIC_GENERATION; K is ignored); GradParams / HessParams: K is the array whose gradient / Hessian
// component is transformed, and is only read.  tl: marks behind the x pass, the y pass and the contiguous pass.
// dst != null: the field goes there instead of the plan's field buffer -- an intermediate of the call (rf_measure_bispectrum's shell
// fields): its moments are not reduced and stats_out is not written.
template <class From>
int generic_c2r(rf_plan* p, const void* K, double* stats_out, Timeline* tl, const From* from, void* dst = nullptr) {
  if (int rc = ensure_g(p)) return rc;
  if (int rc = ensure_g2(p)) return rc;
  HipGenericOps ops{p, p->stream, tl};
  const double scale = inv_cells(p);
  void* W = dst ? dst : p->W.ptr;
  if (from) { if (int rc = generic_c2r_from_seq(ops, p->gdims, *from, K, p->G.ptr, p->G2.ptr, W, scale)) return rc; }
  else if (int rc = generic_c2r_seq(ops, p->gdims, K, p->G.ptr, p->G2.ptr, W, scale)) return rc;
  if (int rc = ops.enter(3)) return rc;
  if (!dst) RF_HIP(launch_reduce_partials(p->partials.get(), p->npartials, stats_out, p->partials.get() + 2 * p->npartials, p->stream));
  return 0;
}

// ONE realisation / transform of a plan that exchanges, on the plan's stream A and the exchange stream E.  E == A when the kz slab goes
// as a whole, and for the direct form with direct_overlap == 0; in sub-slabs what crosses the links -- the grouped send / receive of
// sub-slab c, or its storing y pass -- goes to the exchange stream and runs beside the forward passes of sub-slab c + 1.  Direct: the
// barrier in front keeps the stores away from a peer that still reads (or, in the forward transform's reverse exchange, sends from) its
// receive buffer; the one behind tells every rank that all stores have landed.  The communicator is driven from ONE stream per call: E,
// the all-reduce of the moments too.
// (the timeline: behind the forward half's marks the exchange, the z pass and its moments are the z entry, the all-reduce what is left)
int exchange_c2r(rf_plan* p, const Route& r, const CallDesc& cd, const GenParams& gp, const void* kspace, Timeline* tl) {
  if (r.direct) RF_REQUIRE(p->nranks == 1 || p->comm || p->direct_standin, "virtual ranks linked for the direct exchange run step by step (rf_slab_forward, rf_slab_backward)");
  const int C = r.chunks;
  hipStream_t A = p->stream, E = A;
  if (r.direct || C > 1) {
    RF_HIP(p->comm_stream.create(hipStreamNonBlocking));
    RF_HIP(p->chunk_ev.ensure(C + 1, hipEventDisableTiming));
    if (C > 1 && !(r.direct && p->direct_overlap == 0)) E = p->comm_stream;
  }
  if (E != A) RF_HIP(hop(p->chunk_ev[C], A, E));               // 1. (whatever used R / the communicator before on the plan's stream)
  if (r.direct) { if (int rc = direct_barrier(p, E)) return rc; }                                                   // 2.
  if (int rc = queue_forward(p, r, cd, gp, kspace, p->W.ptr, 0, p->R.ptr, A, E, tl)) return rc;                  // 3.
  if (r.direct) { if (int rc = direct_barrier(p, E)) return rc; }                                                   // 4.
  if (E != A) RF_HIP(hop(p->chunk_ev[C], E, A));                                                                   // 5.
  // 6. the receive buffer is complete for A: the gathering z pass there, then the global (sum, sumsq) -- one 2-double all-reduce on E
  if (int rc = queue_z_slab(p, p->R.ptr, p->W.ptr, p->stats.get(), A)) return rc;
  RF_HIP(mark(tl, rft::Z, A));
  if (p->nranks > 1 && p->comm) {
    if (E != A) RF_HIP(hop(p->chunk_ev[C], A, E));
    RF_NCCL(g_rccl.AllReduce(p->stats.get(), p->stats.get(), 2, ncclFloat64, ncclSum, p->comm, E));
    if (E != A) RF_HIP(hop(p->chunk_ev[C], E, A));
  }
  RF_HIP(tl->end(A));
  p->has.moments_ready(0);
  // 7. a stand-in leaves this rank's own data in the segments (direct: the stores went to its own buffers): no field came out
  if (r.direct ? p->direct_standin : (p->nranks > 1 && !p->comm)) p->has.not_a_field();
  return 0;
}

// one realisation / transform on the plan's stream into the primary buffer; a timed call: every route marks its passes and ends the timeline
int queue_c2r(rf_plan* p, const CallDesc& cd, const GenParams& gp, const void* kspace) {
  Timeline* tl = &p->tl;
  RF_HIP(tl->begin(p->stream, true));
  const Route r = route(p);
  switch (r.kind) {
    case Route::C2C:
      return fail(1, "this call does not apply to an unpacked c2c plan");        // (every entry point has said so before it came here)
    case Route::Generic: {
      // per-kernel times (rf_kernel_ms): start | generation launch | EXTRA | x | X | y | Y | contiguous | Z | reduce | end
      const Source src = source(p, cd.ask(kspace != nullptr));      // (a generic plan runs the exact chain: float64 deviates or none)
      RF_REQUIRE(!src.refused(), src.refusal);
      const bool fused = !kspace && p->fused_generic;  // generation inside the x pass: K and what it holds stay as they are
      if (!kspace && !fused) {                        // rows K,T,R,S into the API-layout buffer first
        if (int rc = ensure_k(p)) return rc;
        RF_HIP(launch_gen_kspace(p->f64, p->K.ptr, gp, p->stream));
        RF_HIP(mark(tl, rft::EXTRA, p->stream));
        p->has.kspace_ready();
        kspace = p->K.ptr;
      }
      if (int rc = generic_c2r(p, kspace, p->stats.get(), tl, fused ? &gp : nullptr)) return rc;
      RF_HIP(tl->end(p->stream));
      break;
    }
    case Route::Single:          // one GPU: x pass, then the y / z passes (slab by slab on large grids)
      if (int rc = queue_xyz(p, cd, gp, kspace, p->W.ptr, p->stream, p->stats.get(), tl)) return rc;
      break;
    case Route::Replicated:
      if (int rc = queue_xy(p, cd, gp, kspace, p->W.ptr, p->stream, tl)) return rc;
      if (int rc = replicated_z(p, 0, 1, tl)) return rc;
      RF_HIP(tl->end(p->stream));
      break;
    case Route::Exchange:
      return exchange_c2r(p, r, cd, gp, kspace, tl);
  }
  p->has.field_ready(p->W.ptr, 0);
  return 0;
}

template <typename T> int upload_twiddles(DevBuf<>& dst, int n) {
  auto w = make_twiddles<T>(n);
  hipError_t e = dst.reserve(w.size() * sizeof(cplx<T>));
  if (e != hipSuccess) return fail(2, std::string("hipMalloc twiddles: ") + hipGetErrorString(e));
  e = hipMemcpy(dst.ptr, w.data(), w.size() * sizeof(cplx<T>), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(2, std::string("hipMemcpy twiddles: ") + hipGetErrorString(e));
  return 0;
}

// What rf_plan_create and rf_plan_create_c2c share, in the order of the allocations: the plan's stream, the field buffer W (and R on
// multi-rank plans), the twiddle tables of the three axes, the workspace of a packed plan (p->npartials is set), the timing events
int create_common(rf_plan* p, bool packed) {
  hipError_t e;
  if ((e = p->own_stream.create(hipStreamNonBlocking)) != hipSuccess) return fail(2, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  p->stream = p->own_stream;
  if ((e = p->W.reserve(p->w_bytes)) != hipSuccess || (p->nranks > 1 && (e = p->R.reserve(p->w_bytes)) != hipSuccess))
    return fail(2, std::string("hipMalloc field buffer: ") + hipGetErrorString(e));
  const int n[3] = {p->nx, p->ny, p->nz};
  DevBuf<>* tw[3] = {&p->tw_x, &p->tw_y, &p->tw_z};
  for (int a = 0; a < 3; ++a)
    if (int rc = p->f64 ? upload_twiddles<double>(*tw[a], n[a]) : upload_twiddles<float>(*tw[a], n[a])) return rc;
  if (packed &&
      ((e = p->partials.reserve((2 * p->npartials + 512) * sizeof(double))) != hipSuccess ||
       (e = p->stats.reserve(2 * 64 * sizeof(double))) != hipSuccess ||
       (e = p->coll_scratch.reserve(4 * sizeof(double))) != hipSuccess ||      // [0..1] host-side all-reduces, [2..3] the direct exchange's barriers
       (e = p->kx2.reserve(p->nx * sizeof(double))) != hipSuccess ||
       (e = p->ky2.reserve(p->ny * sizeof(double))) != hipSuccess ||
       (e = p->kz2.reserve((p->nzc + 1) * sizeof(double))) != hipSuccess ||
       (e = p->ztab.reserve(2 * p->nz * sizeof(double))) != hipSuccess))
    return fail(2, std::string("hipMalloc workspace: ") + hipGetErrorString(e));
  if ((e = p->tl.ev.ensure(6, hipEventDefault)) != hipSuccess) return fail(2, std::string("hipEventCreate: ") + hipGetErrorString(e));      // (start, end and a whole-grid call's four marks; more on demand)
  return 0;
}

int shape_check(int nx, int ny, int nz, int f64, std::string* why, int nranks = 1) {
  auto bad = [&](const std::string& m) { if (why) *why = m; return 1; };
  if (nx <= 0 || ny <= 0 || nz <= 0) return bad("grid dimensions must be positive");
  if (nz % 4) return bad("nz must be a multiple of 4 (packed layout, transform.py:53-56)");
  if (!col_size_supported(nx) || !col_size_supported(ny))
    return bad("HIP path needs nx, ny in {8,16,...,2048} (powers of two)");
  if (!row_size_supported(nz / 2)) return bad("HIP path needs nz in {16,32,...,2048} (powers of two)");
  const long long nzc = nz / 2;
  if (nranks > 1 && (nx % nranks || nzc % nranks || (nzc / nranks) % 2))
    return bad("nx and nz/2 must be divisible by the number of ranks (and nz/(2*ranks) must be even)");
  const long long nzl = nzc / nranks;
  if (((long long)ny * nzl) % col_tile_cols(f64, nx)) return bad("ny*nz/(2*ranks) is not a multiple of the x-pass tile width");
  if (((long long)nx * nzl) % col_tile_cols(f64, ny)) return bad("nx*nz/(2*ranks) is not a multiple of the y-pass tile width");
  return 0;
}

}  // namespace rfc

extern "C" {

int rf_version(void) { return RF_ABI_VERSION; }

unsigned rf_abi_features(void) {
  return RF_FEATURE_REALISE | RF_FEATURE_R2C | RF_FEATURE_C2C | RF_FEATURE_LOGNORMAL | RF_FEATURE_POTENTIAL | RF_FEATURE_LENSING |
         RF_FEATURE_MT19937 | RF_FEATURE_MT19937_SHARED | RF_FEATURE_MULTI_RANK | RF_FEATURE_GENERIC_SHAPES | RF_FEATURE_EXCHANGE_CHUNKS |
         RF_FEATURE_DIRECT_EXCHANGE | RF_FEATURE_DIAGNOSTICS | RF_FEATURE_GENERIC_FUSED | RF_FEATURE_GRADIENT | RF_FEATURE_POWER_MEASURE | RF_FEATURE_LPT2 |
         RF_FEATURE_PARTICLES | RF_FEATURE_POWER_MULTIPOLES | RF_FEATURE_PARTICLES_GATHER | RF_FEATURE_PARTICLES_TSC |
         RF_FEATURE_PARTICLES_INTERLACE | RF_FEATURE_BISPECTRUM;
}

const char* rf_last_error(void) { return g_err.c_str(); }

int rf_device_count(int* count) {
  RF_REQUIRE(count != nullptr, "count is null");
  RF_HIP(hipGetDeviceCount(count));
  return 0;
}

// 1: tiled power-of-two kernels; 2: the generic path for other even shapes (rf_generic.h); 0: not supported
int rf_shape_supported(int nx, int ny, int nz) {
  if (shape_check(nx, ny, nz, 0, nullptr) == 0 && shape_check(nx, ny, nz, 1, nullptr) == 0) return 1;
  GenericAxis a, b, c;
  return generic_shape(nx, ny, nz, 0, a, b, c) ? 2 : 0;          // (complex128 plans: axes up to 4096 -- rf_plan_create says so)
}

// the same for one dtype: exactly what rf_plan_create on one rank accepts (complex128 plans: generic axes up to 4096)
int rf_shape_supported_dtype(int nx, int ny, int nz, int dtype) {
  if (dtype != RF_F32 && dtype != RF_F64) return 0;
  if (shape_check(nx, ny, nz, dtype, nullptr) == 0) return 1;
  GenericAxis a, b, c;
  return generic_shape(nx, ny, nz, dtype == RF_F64, a, b, c) ? 2 : 0;
}

int rf_plan_create(rf_plan** out, int nx, int ny, int nz, int dtype, int device, int nranks, int rank) {
  RF_REQUIRE(out != nullptr, "plan pointer is null");
  *out = nullptr;
  RF_REQUIRE(dtype == RF_F32 || dtype == RF_F64, "dtype must be RF_F32 or RF_F64");
  std::string why;
  RF_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "invalid nranks/rank");
  GenericDims gd;
  bool generic = false;
  if (shape_check(nx, ny, nz, dtype, &why, nranks)) {
    generic = nranks == 1 && generic_dims(nx, ny, nz, dtype == RF_F64, true, gd);
    if (!generic)
      return fail(1, "unsupported shape: " + why + (nranks == 1 ? std::string(" (and not an even shape whose axes fit one line of the LDS -- ") + (dtype == RF_F64 ? "4096 points on complex128 plans" : "8192 points on complex64 plans") + " -- or split into two factors that do, either: rf_shape_supported_dtype)" : ""));
  }
  RF_HIP(hipSetDevice(device));
  rf_plan* p = new rf_plan();
  p->generic = generic;
  if (generic) { p->gdims = gd; p->gax = gd.ax; p->gay = gd.ay; p->gaz = gd.az; }
  p->nx = nx; p->ny = ny; p->nz = nz; p->nzc = nz / 2; p->f64 = dtype; p->device = device;
  p->nranks = nranks; p->rank = rank;
  p->csize = dtype ? 16 : 8;
  p->nxl = nx / nranks; p->nzl = p->nzc / nranks; p->kz0 = rank * p->nzl;
  p->w_bytes = (size_t)nx * ny * p->nzl * p->csize;       // == nxl * ny * nzc: the local share of the field
  p->k_bytes = (size_t)nx * ny * (p->nzl + 1) * p->csize;    // side arrays: this rank's planes + the Nyquist plane
  // float32: an even pitch (nzl is even), so that the fused store writes 16-byte aligned cell pairs; on large grids 64 cells
  // beyond the row instead of 2 -- the time of the two strided store streams of rf_realise_potential depends on where the
  // allocator puts the two arrays (tools/frag_probe.py, 1024^3: 5.6 / 6.8 / 6.9 ms in three allocation histories with pitch
  // nz/2 + 2; 5.5 / 6.1 / 6.0 ms with nz/2 + 64), which a row stride further from the field's 4 MiB softens
  p->ppitch = dtype ? (int)p->nzl + 1 : (int)p->nzl + (p->nzl >= 256 ? 64 : 2);
  p->p_bytes = (size_t)nx * ny * p->ppitch * p->csize;
  auto cleanup = [&](int rc) { delete p; return rc; };
  hipError_t e;
  p->npartials = generic ? (gd.lz.split() ? 1024 : generic_row_blocks(dtype, gd.az, (long long)nx * ny))      // (long rows: the moments are a pass of their own, 1024 blocks)
               : nranks > 1 ? row_c2r_tiles(dtype, p->nzc, (long long)p->nxl * ny) : row_c2r_tiles(dtype, p->nzc, (long long)nx * ny);
  if (int rc = create_common(p, true)) return cleanup(rc);
  // function attributes (dynamic LDS above 64 KB) are set here, never inside a graph capture
  if (!generic && (e = prepare_packed_kernels(dtype, nx, ny, (int)p->nzc)) != hipSuccess)
    return cleanup(fail(2, std::string("kernel preparation: ") + hipGetErrorString(e)));
  *out = p;
  return 0;
}

// Unpacked c2c plan (transform.py:207-213,266-270): one buffer [nx][ny][nz] complex, transformed in place.
int rf_plan_create_c2c(rf_plan** out, int nx, int ny, int nz, int dtype, int device) {
  RF_REQUIRE(out != nullptr, "plan pointer is null");
  *out = nullptr;
  RF_REQUIRE(dtype == RF_F32 || dtype == RF_F64, "dtype must be RF_F32 or RF_F64");
  bool generic = !col_size_supported(nx) || !col_size_supported(ny) || !rowc_size_supported(nz);
  if (!generic) {
    const int tcx = col_tile_cols(dtype, nx), tcy = col_tile_cols(dtype, ny);
    generic = ((long long)ny * nz) % tcx || ((long long)nx * nz) % tcy;      // too few columns for a tile
  }
  GenericDims gd;
  if (generic && !generic_dims(nx, ny, nz, dtype == RF_F64, false, gd))
    return fail(1, "unsupported shape for a c2c plan: nx, ny, nz must be even, and every axis must fit one line of the LDS (8192 points complex64 / 4096 complex128) or split into two factors that do");
  RF_HIP(hipSetDevice(device));
  rf_plan* p = new rf_plan();
  p->generic = generic;
  if (generic) { p->gdims = gd; p->gax = gd.ax; p->gay = gd.ay; p->gaz = gd.az; }
  p->nx = nx; p->ny = ny; p->nz = nz; p->nzc = nz / 2; p->f64 = dtype; p->device = device;
  p->nranks = 1; p->rank = 0; p->csize = dtype ? 16 : 8; p->nxl = nx; p->nzl = p->nzc; p->kz0 = 0;
  p->unpacked = true;
  p->w_bytes = (size_t)nx * ny * nz * p->csize;
  p->k_bytes = 0;
  auto cleanup = [&](int rc) { delete p; return rc; };
  hipError_t e;
  if (int rc = create_common(p, false)) return cleanup(rc);
  const ColGeom gx{(long long)ny * nz, 0, (long long)ny * nz}, gy{nz, (long long)ny * nz, nz};
  if (!generic && (!col_plain_addressable(dtype, nx, gx) || !col_plain_addressable(dtype, ny, gy)))
    return cleanup(fail(1, "unsupported shape for a c2c plan: an axis shorter than 1024 with rows more than 4 GiB apart "
                           "(32-bit lane offsets); make that axis >= 1024 or the others smaller"));
  for (int dir = -1; dir <= 1 && !generic; dir += 2)
    if ((e = prepare_c2c_kernels(dtype, nx, ny, nz, dir)) != hipSuccess)
      return cleanup(fail(2, std::string("kernel preparation: ") + hipGetErrorString(e)));
  *out = p;
  return 0;
}

int rf_upload_c(rf_plan* p, const void* host) {
  RF_REQUIRE(p && host, "null argument");
  RF_REQUIRE(p->unpacked, "rf_upload_c is for plans made by rf_plan_create_c2c");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(p->W.ptr, host, p->w_bytes, hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

int rf_download_c(rf_plan* p, void* host) {
  RF_REQUIRE(p && host, "null argument");
  RF_REQUIRE(p->unpacked, "rf_download_c is for plans made by rf_plan_create_c2c");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(host, p->W.ptr, p->w_bytes, hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

// direction = -1: forward, unnormalised (np.fft.fftn); +1: inverse with numpy's 1/(nx ny nz) (np.fft.ifftn)
int rf_execute_c2c(rf_plan* p, int direction) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(p->unpacked, "rf_execute_c2c is for plans made by rf_plan_create_c2c");
  RF_REQUIRE(direction == 1 || direction == -1, "direction must be +1 (inverse) or -1 (forward)");
  RF_HIP(hipSetDevice(p->device));
  const long long nz = p->nz;
  const ColGeom gx{(long long)p->ny * nz, 0, (long long)p->ny * nz}, gy{nz, (long long)p->ny * nz, nz};
  const double scale = direction > 0 ? inv_cells(p) : 1.0;
  RF_HIP(p->tl.begin(p->stream, false));
  if (p->generic) {
    if (generic_any_long(p)) RF_HIP(p->G.reserve(p->w_bytes));        // scratch of the four-step form
    HipGenericOps ops{p, p->stream};
    if (int rc = generic_c2c_seq(ops, p->gdims, p->W.ptr, p->G.ptr, direction, scale)) return rc;
  } else {
    RF_HIP(launch_col_plain(p->f64, p->nx, direction, p->W.ptr, gx, (long long)p->ny * nz, p->tw_x.ptr, p->stream));
    RF_HIP(launch_col_plain(p->f64, p->ny, direction, p->W.ptr, gy, (long long)p->nx * nz, p->tw_y.ptr, p->stream));
    RF_HIP(launch_row_c2c(p->f64, (int)nz, direction, p->W.ptr, (long long)p->nx * p->ny, scale, p->tw_z.ptr, p->stream));
  }
  RF_HIP(p->tl.end(p->stream));
  return 0;
}

// (the owning members free everything; the streams are the first members of rf_plan and so the last to go)
int rf_plan_destroy(rf_plan* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  for (hipStream_t s : {p->stream, (hipStream_t)p->comm_stream, (hipStream_t)p->dl_stream, (hipStream_t)p->aux_stream})
    if (s) (void)hipStreamSynchronize(s);
  drop_graphs(p);
  if (p->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(p->comm);
  for (void* m : p->ipc_open) (void)hipIpcCloseMemHandle(m);
  delete p;
  return 0;
}

int rf_plan_nbytes(rf_plan* p, size_t* nbytes) {
  RF_REQUIRE(p && nbytes, "null argument");
  *nbytes = p->W.bytes + p->R.bytes + p->W2.bytes + p->R2.bytes + p->X.bytes + p->K.bytes + p->P.bytes + p->L.bytes + p->Q.bytes + p->A.bytes + p->PG.bytes +
            p->G.bytes + p->G2.bytes + p->noise.bytes + p->mt.scratch.bytes + p->mp_buf.bytes + p->KS.bytes +      // (+ resident deviates and the replay's scratch runs)
            p->bs_mask.bytes + p->bs_fields.bytes + p->bs_part.bytes;
  return 0;
}

int rf_diag_live_resources(size_t* device_bytes, int* events, int* streams) {
  RF_REQUIRE(device_bytes && events && streams, "null argument");
  *device_bytes = rfo::live().device_bytes; *events = rfo::live().events; *streams = rfo::live().streams;
  return 0;
}

int rf_diag_generation_path(rf_plan* p, int* fast) {
  RF_REQUIRE(p && fast, "null argument");
  *fast = source(p, SourceAsk()).fast() ? 1 : 0;      // what a NATIVE x pass would run
  return 0;
}

int rf_plan_set_flag(rf_plan* p, int flag, int value) {
  RF_REQUIRE(p, "null plan");
  if (flag == RF_FLAG_FUSED_GENERIC_GENERATION) {  // the x pass generates the half spectrum it transforms (rf_generic.h generic_c2r_from_seq)
    RF_REQUIRE(p->generic && !p->unpacked && p->nranks == 1,
               "RF_FLAG_FUSED_GENERIC_GENERATION is for packed single-rank plans on the generic kernels (shapes that are not powers of two): "
               "the tiled kernels always generate inside their x pass");
    RF_HIP(hipStreamSynchronize(p->stream));
    p->fused_generic = value != 0;
    return 0;
  }
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(flag == RF_FLAG_EXACT_GENERATION || flag == RF_FLAG_FORCE_SLAB_PATH || flag == RF_FLAG_REPLICATED_GENERATION ||
             flag == RF_FLAG_TRANSPOSED_INTERMEDIATE || flag == RF_FLAG_YZ_SLAB_PLANES || flag == RF_FLAG_EXCHANGE_CHUNKS, "unknown flag");
  RF_HIP(hipStreamSynchronize(p->stream));
  if (p->comm_stream) RF_HIP(hipStreamSynchronize(p->comm_stream));
  if (flag == RF_FLAG_EXCHANGE_CHUNKS) {         // sub-slabs of the exchange: 1 (or 0) = the whole kz slab at once
    const int C = value <= 1 ? 1 : value;
    RF_REQUIRE(!p->generic && !p->unpacked, "RF_FLAG_EXCHANGE_CHUNKS is for packed plans on the tiled kernels");
    RF_REQUIRE((C & (C - 1)) == 0 && p->nzl % C == 0, "the number of exchange chunks must be a power of two that divides nz / (2 ranks)");
    const long long nzc_ = p->nzl / C;
    RF_REQUIRE(C == 1 || (nzc_ % 2 == 0 && ((long long)p->ny * nzc_) % col_tile_cols(p->f64, p->nx) == 0 &&
                          ((long long)p->ny * nzc_) % col_gen_tile_cols(p->f64, p->nx) == 0 && ((long long)p->nx * nzc_) % col_tile_cols(p->f64, p->ny) == 0),
               "too many exchange chunks for this grid: a sub-slab must hold an even number of planes and whole tiles of the x and y passes");
    RF_REQUIRE(!p->direct || col_direct_supported(p->f64, p->ny, nzc_),
               "too many exchange chunks for the direct exchange: a y-pass tile would straddle two x planes");
    p->xchunks = C;
    drop_graphs(p);
    p->has.not_a_field();                        // (the buffers' layout between the passes changes; nothing resident survives it)
    if (p->direct) return rebuild_peer_tab(p);
    return 0;
  }
  if (flag == RF_FLAG_YZ_SLAB_PLANES) {          // -1 automatic, 0 whole-grid passes, > 0 x planes per slab
    p->yz_slab = value;
    drop_graphs(p);
    return 0;
  }
  if (flag == RF_FLAG_TRANSPOSED_INTERMEDIATE) {
    p->xposed = value != 0;
    drop_graphs(p);
    if (!p->xposed) RF_HIP(p->X.release());
    return 0;
  }
  if (flag == RF_FLAG_REPLICATED_GENERATION) {
    RF_REQUIRE(p->nranks > 1, "RF_FLAG_REPLICATED_GENERATION is for multi-rank plans");
    RF_REQUIRE(!value || col_replicate_supported(p->f64, p->nx, p->nranks),
               "replicated generation is not available for this shape (nx too small for the number of ranks, or float64 with nx = 2048)");
    p->replicate = value != 0;
    return 0;
  }
  if (flag == RF_FLAG_FORCE_SLAB_PATH) {
    RF_REQUIRE(p->nranks == 1, "RF_FLAG_FORCE_SLAB_PATH is for single-rank plans");
    RF_REQUIRE(!p->generic, "RF_FLAG_FORCE_SLAB_PATH needs power-of-two axes");
    if (value) RF_HIP(p->R.reserve(p->w_bytes));
    p->force_slab = value != 0;
    drop_graphs(p);
    return 0;
  }
  p->exact_gen = value != 0;
  drop_graphs(p);
  return 0;
}

int rf_plan_set_stream(rf_plan* p, void* hip_stream) {
  RF_REQUIRE(p, "null plan");
  RF_HIP(hipStreamSynchronize(p->stream));
  p->stream = hip_stream ? (hipStream_t)hip_stream : p->own_stream;
  drop_graphs(p);
  return 0;
}

int rf_set_kgrid(rf_plan* p, const double* kx2, const double* ky2, const double* kz2) {
  RF_REQUIRE(p && kx2 && ky2 && kz2, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(p->kx2.get(), kx2, p->nx * sizeof(double), hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipMemcpyAsync(p->ky2.get(), ky2, p->ny * sizeof(double), hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipMemcpyAsync(p->kz2.get(), kz2, (p->nzc + 1) * sizeof(double), hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  p->h_kx2.assign(kx2, kx2 + p->nx); p->h_ky2.assign(ky2, ky2 + p->ny); p->h_kz2.assign(kz2, kz2 + p->nzc + 1);
  p->have_kgrid = true;
  return build_fast(p);
}

int rf_set_power(rf_plan* p, const double* log10k, const double* sigma, int n) {
  RF_REQUIRE(p && log10k && sigma, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(n >= 2, "power table needs at least 2 rows");
  for (int i = 0; i + 1 < n; ++i) RF_REQUIRE(log10k[i + 1] > log10k[i], "log10k must be strictly increasing");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipStreamSynchronize(p->stream));
  SigmaTableHost t;
  build_sigma_table(log10k, sigma, n, t);
  p->have_power = false;
  RF_HIP(p->xt.release()); RF_HIP(p->st.release()); RF_HIP(p->sl.release()); RF_HIP(p->bin.release());      // (always fresh tables)
  RF_HIP(p->xt.reserve(n * sizeof(double)));
  RF_HIP(p->st.reserve(n * sizeof(double)));
  RF_HIP(p->sl.reserve(t.sl.size() * sizeof(double)));
  RF_HIP(p->bin.reserve(t.bin.size() * sizeof(int)));
  RF_HIP(hipMemcpy(p->xt.get(), t.xt.data(), n * sizeof(double), hipMemcpyHostToDevice));
  RF_HIP(hipMemcpy(p->st.get(), t.st.data(), n * sizeof(double), hipMemcpyHostToDevice));
  RF_HIP(hipMemcpy(p->sl.get(), t.sl.data(), t.sl.size() * sizeof(double), hipMemcpyHostToDevice));
  RF_HIP(hipMemcpy(p->bin.get(), t.bin.data(), t.bin.size() * sizeof(int), hipMemcpyHostToDevice));
  p->nt = n; p->nbins = (int)t.bin.size(); p->x0 = t.x0; p->inv_dx = t.inv_dx;
  p->have_power = true;
  p->h_tab = t;
  return build_fast(p);
}

int rf_generate(rf_plan* p, uint64_t seed, int mode, const double* noise_host) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
  RF_REQUIRE(mode == RF_NOISE_NATIVE || mode == RF_NOISE_EXTERNAL || mode == RF_NOISE_RESIDENT, "invalid noise mode");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_k(p)) return rc;        // a kz-slab rank holds (and generates) its own planes + the Nyquist plane
  if (int rc = upload_noise(p, mode, noise_host)) return rc;
  const Source src = source(p, SourceAsk::fill_k(mode));      // the exact chain into K: Philox, or float64 deviates
  RF_REQUIRE(!src.refused(), src.refusal);
  RF_HIP(launch_gen_kspace(p->f64, p->K.ptr, make_gen(p, seed, mode), p->stream));
  if (mode == RF_NOISE_EXTERNAL) RF_HIP(hipStreamSynchronize(p->stream));  // host noise buffer may be released by the caller
  p->has.kspace_ready();
  return 0;
}

int rf_execute_c2r(rf_plan* p) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->K.ptr && p->has.kspace(), "no k-space data: call rf_generate or rf_upload_k first");
  RF_REQUIRE(!route(p).replicates(), "replicated-generation plans have no distributed k-space buffer");
  RF_HIP(hipSetDevice(p->device));
  return queue_c2r(p, CallDesc(), make_gen(p, 0, RF_NOISE_NATIVE), p->K.ptr);
}

}  // extern "C"
namespace rfc {
// multi-rank forward transform, x-slab half: z pass on the local rows, in place, then the rows cut into the P send blocks
// [nxl][ny][nzl] of R (block g = the kz planes of rank g) -- the reverse of what the gathering z pass reads
int queue_r2c_slab_rows(rf_plan* p, hipStream_t s) {
  const long long nrows = (long long)p->nxl * p->ny;
  RF_HIP(launch_row_r2c(p->f64, (int)p->nzc, p->W.ptr, nrows, p->tw_z.ptr, s));
  const size_t seg = (size_t)p->nzl * p->csize, blk = (size_t)nrows * seg;
  for (int g = 0; g < p->nranks; ++g)
    RF_HIP(hipMemcpy2DAsync((char*)p->R.ptr + g * blk, seg, (const char*)p->W.ptr + g * seg, (size_t)p->nzc * p->csize, seg, (size_t)nrows,
                            hipMemcpyDeviceToDevice, s));
  return 0;
}
// kz-slab half: forward y and x passes on [nx][ny][nzl] (the blocks as they arrived: x is the slowest axis), then the side array
int queue_r2c_slab_cols(rf_plan* p, hipStream_t s) {
  const long long nzl = p->nzl;
  const ColGeom gx{(long long)p->ny * nzl, 0, (long long)p->ny * nzl}, gy{nzl, (long long)p->ny * nzl, nzl};
  RF_HIP(launch_col_plain(p->f64, p->ny, -1, p->W.ptr, gy, (long long)p->nx * nzl, p->tw_y.ptr, s));
  RF_HIP(launch_col_plain(p->f64, p->nx, -1, p->W.ptr, gx, (long long)p->ny * nzl, p->tw_x.ptr, s));
  RF_HIP(launch_unpack_kspace(p->f64, p->W.ptr, p->K.ptr, p->nx, p->ny, (int)nzl, p->kz0, s));
  p->has.field_consumed();    // the field buffer now holds packed k space
  p->has.kspace_ready();
  return 0;
}
// single-rank forward transform of the field in W.  Generic plans: rows -> half spectrum in K, then the y and x forward passes
// (rf_generic.h generic_r2c_seq); W is untouched.  Tiled plans: the three passes in place in W, then (unpack) the API-layout array K;
// without it W is left packed (slot kz = 0 = A0 + i A_nyq), K and what it holds as they were (rf_measure_power reads W directly).
// spectrum: where the half spectrum goes when it is not K (the stash of an interlaced paint: K and what it holds stay as they were)
int queue_r2c_single(rf_plan* p, bool unpack, void* spectrum) {
  const long long nzc = p->nzc;
  const ColGeom gx{(long long)p->ny * nzc, 0, (long long)p->ny * nzc}, gy{nzc, (long long)p->ny * nzc, nzc};
  if (p->generic) {
    if (int rc = ensure_k(p)) return rc;
    if (generic_any_long(p)) { if (int rc = ensure_g(p)) return rc; if (int rc = ensure_g2(p)) return rc; }
    HipGenericOps ops{p, p->stream};
    if (int rc = generic_r2c_seq(ops, p->gdims, p->W.ptr, spectrum ? spectrum : p->K.ptr, p->G.ptr, p->G2.ptr)) return rc;
    if (!spectrum) p->has.kspace_ready();            // the real field in W is untouched on this path
    return 0;
  }
  if (unpack) { if (int rc = ensure_k(p)) return rc; }
  RF_HIP(launch_row_r2c(p->f64, (int)nzc, p->W.ptr, (long long)p->nx * p->ny, p->tw_z.ptr, p->stream));     // z, in place
  RF_HIP(launch_col_plain(p->f64, p->ny, -1, p->W.ptr, gy, (long long)p->nx * nzc, p->tw_y.ptr, p->stream));   // y forward
  RF_HIP(launch_col_plain(p->f64, p->nx, -1, p->W.ptr, gx, (long long)p->ny * nzc, p->tw_x.ptr, p->stream));   // x forward
  p->has.field_consumed();    // the field buffer now holds packed k space
  if (unpack) {
    RF_HIP(launch_unpack_kspace(p->f64, p->W.ptr, spectrum ? spectrum : p->K.ptr, p->nx, p->ny, (int)nzc, 0, p->stream));
    if (!spectrum) p->has.kspace_ready();
  }
  return 0;
}
}  // namespace rfc
extern "C" {

int rf_execute_r2c(rf_plan* p) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->has.field_in(p->W.ptr), "no real-space field on the device: call rf_upload_real (or a c2r) first");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_k(p)) return rc;
  if (p->nranks > 1) {
    // transform.py:278-301 on x-slab / kz-slab ranks: rows, the all-to-all in the other direction (block g of R -> rank g,
    // arriving as block h of W: the same grouped send / receive with the buffers swapped), columns
    RF_REQUIRE(route(p).exchanges(), "the multi-rank forward transform runs on the tiled kernels of exchange-mode plans");
    RF_HIP(p->tl.begin(p->stream, false));
    if (int rc = queue_r2c_slab_rows(p, p->stream)) return rc;
    if (int rc = queue_exchange_rccl(p, p->R.ptr, p->W.ptr, p->stream, -1, true)) return rc;
    if (int rc = queue_r2c_slab_cols(p, p->stream)) return rc;
    RF_HIP(p->tl.end(p->stream));
    return 0;
  }
  RF_HIP(p->tl.begin(p->stream, false));
  if (int rc = queue_r2c_single(p, true, nullptr)) return rc;
  RF_HIP(p->tl.end(p->stream));
  return 0;
}

int rf_realise(rf_plan* p, uint64_t seed, int mode, const double* noise_host) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
  RF_REQUIRE(mode == RF_NOISE_NATIVE || mode == RF_NOISE_EXTERNAL || mode == RF_NOISE_RESIDENT, "invalid noise mode");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = upload_noise(p, mode, noise_host)) return rc;
  if (int rc = queue_c2r(p, CallDesc(mode), make_gen(p, seed, mode), nullptr)) return rc;
  if (mode == RF_NOISE_EXTERNAL) RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

// calculate_newtonian_potential (generate.py:333-343) WITHOUT a stored potential: the inverse transform of scale * delta(k) / k^2,
// with delta(k) regenerated inside the x pass exactly as rf_realise(seed, mode) generates it -- the native generator is keyed by
// (seed, cell), the replayed reference stream is still resident -- so generate_delta_field(save_potential=True) need not write
// 4.3 GB per 1024^3 "in case" and the later load + transform reads nothing.  Every cell is rounded as its stored copy and the
// scaled copy of that would be.  Needs the fast generation pass (rf_can_regenerate_potential); returns the real field in place of
// the current one, like rf_load_potential + rf_execute_c2r.
int rf_can_regenerate_potential(rf_plan* p, int mode) {
  if (!p || (mode != RF_NOISE_NATIVE && mode != RF_NOISE_EXTERNAL && mode != RF_NOISE_RESIDENT)) return 0;
  return source(p, SourceAsk::x_pass(false, mode, SourceAsk::Emitted)).emits_potential() ? 1 : 0;      // what rf_realise_scaled_potential's x pass will ask
}

int rf_realise_scaled_potential(rf_plan* p, uint64_t seed, int mode, double scale, const double* factor_z) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
  RF_REQUIRE(rf_can_regenerate_potential(p, mode), "this plan / noise mode stores its potential (rf_realise_potential): nothing to regenerate from");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = upload_noise(p, mode, nullptr)) return rc;
  CallDesc cd(mode);
  cd.emit_potential = true;
  cd.emit_pscale = p->f64 ? scale : (double)(float)scale;
  // the light-cone factor per plane z (generate.py:344-347): in the z pass's own store where the plan runs the plain single-rank
  // passes, else by the sweep rf_scale_z would make -- the same two roundings either way
  // (decided from the plan's FLAG: the blocked intermediate X is allocated lazily inside queue_c2r, and its gathering z pass has no
  // per-z factor -- testing p->X here dropped the factor on the first call after RF_FLAG_TRANSPOSED_INTERMEDIATE was set)
  if (int rc = ensure_x(p)) return rc;
  const bool fuse_z = factor_z && route(p).single() && !xpose_ok(p);
  if (factor_z) RF_HIP(hipMemcpyAsync(p->ztab.get(), factor_z, (size_t)p->nz * sizeof(double), hipMemcpyHostToDevice, p->stream));
  cd.zscale = fuse_z ? p->ztab.get() : nullptr;
  if (int rc = queue_c2r(p, cd, make_gen(p, seed, mode), nullptr)) return rc;
  if (factor_z && !fuse_z) {
    RF_HIP(launch_affine_z(p->f64, p->has.where(), (long long)p->nxl * p->ny, p->nz, p->ztab.get(), 0.0, p->stream));
    p->has.field_modified();
  }
  if (factor_z) RF_HIP(hipStreamSynchronize(p->stream));     // (factor_z is the caller's memory)
  return 0;
}

}  // extern "C"
namespace rfc {
// mean and standard deviation of a field of the plan from its (sum, sumsq) pair
void mean_std(const rf_plan* p, const double* st, double* mean, double* std_out) {
  const double cnt = (double)p->nx * p->ny * p->nz;
  const double m = st[0] / cnt;
  const double v = st[1] / cnt - m * m;
  if (mean) *mean = m;
  if (std_out) *std_out = v > 0 ? std::sqrt(v) : 0.0;
}

// the rms of the first n realisations of a batch, from their pairs in `stats` (waits for the plan's stream)
int rms_from_stats(rf_plan* p, int n, double* rms_out) {
  std::vector<double> st(2 * (size_t)n);
  RF_HIP(hipMemcpyAsync(st.data(), p->stats.get(), st.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  for (int i = 0; i < n; ++i) mean_std(p, &st[2 * i], nullptr, rms_out + i);
  return 0;
}

// generate_delta_field(save_potential=True) (generate.py:191-219): the field as rf_realise, plus delta(k) / k^2 in the
// plan's potential buffer.  With the native generator (or resident float32 deviates) the potential is a second store
// stream of the generation pass; every other case runs the unfused sequence generate -> save_potential -> c2r.
// whole = false stops after the y pass (the slab pipeline's forward half, rf_slab_forward_ex)
int potential_forward(rf_plan* p, uint64_t seed, int mode, const double* noise_host, bool whole) {
  RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
  RF_REQUIRE(mode == RF_NOISE_NATIVE || mode == RF_NOISE_EXTERNAL || mode == RF_NOISE_RESIDENT, "invalid noise mode");
  RF_REQUIRE(!route(p).replicates(), "replicated-generation plans keep no k-space potential: clear RF_FLAG_REPLICATED_GENERATION");
  RF_HIP(hipSetDevice(p->device));
  // fused: delta(k) / k^2 is a second store stream of the generation pass -- native generator (float32 and float64 plans)
  // or resident float32 deviates (float32 plans): the x pass's own decision, asked what its call will ask
  if (!source(p, SourceAsk::x_pass(false, mode, SourceAsk::Stored)).stores_potential()) {
    if (int rc = rf_generate(p, seed, mode, noise_host)) return rc;
    if (int rc = rf_save_potential(p)) return rc;
    if (whole) return rf_execute_c2r(p);
    return queue_xy(p, CallDesc(), make_gen(p, 0, RF_NOISE_NATIVE), p->K.ptr, p->W.ptr, p->stream, nullptr);
  }
  if (int rc = ensure_p(p)) return rc;
  p->has.potential2_stale();                         // (P is rewritten: a second-order potential made from the old one is stale)
  CallDesc cd(mode);
  cd.pot_target = p->P.ptr;
  const GenParams gp = make_gen(p, seed, mode);
  return whole ? queue_c2r(p, cd, gp, nullptr) : queue_xy(p, cd, gp, nullptr, p->W.ptr, p->stream, nullptr);
}
}  // namespace rfc
extern "C" {

int rf_realise_potential(rf_plan* p, uint64_t seed, int mode, const double* noise_host) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  return potential_forward(p, seed, mode, noise_host, true);
}

// issue the n realisations of a batch on the plan's stream (under stream capture)
static int batch_issue(rf_plan* p, int n) {
  for (int i = 0; i < n; ++i) {
    GenParams gp = make_gen(p, 0, RF_NOISE_NATIVE);
    gp.seed_dev = p->seeds_dev.get() + i;
    if (int rc = queue_xyz(p, CallDesc(), gp, nullptr, p->W.ptr, p->stream, p->stats.get() + 2 * i, nullptr)) return rc;
  }
  return 0;
}

// Capture the whole batch as ONE graph: realisation i reads seed[i] from device memory and leaves its
// (sum, sumsq) in stats[2i].  (Two-stream pipelining of consecutive realisations was measured on
// MI355X and gave nothing: an x-pass and a y-pass kernel do not co-execute profitably -- DESIGN.md.)
static int batch_prepare(rf_plan* p, int n) {
  RF_REQUIRE(n >= 1, "need at least one seed");
  RF_REQUIRE(p->nranks == 1, "graph-captured batches are single-GPU; loop rf_realise on multi-GPU plans");
  RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
  RF_HIP(hipSetDevice(p->device));
  if (p->seeds_dev.bytes < n * sizeof(uint64_t) || p->stats.bytes < 2 * n * sizeof(double)) {
    // device arrays are baked into the captured graphs: grow them (generously) and start over -- BOTH, each at exactly `cap` entries
    RF_HIP(hipStreamSynchronize(p->stream));
    drop_graphs(p);
    const size_t cap = n > 64 ? n : 64;
    RF_HIP(p->seeds_dev.release());
    RF_HIP(p->seeds_dev.reserve(cap * sizeof(uint64_t)));
    RF_HIP(p->stats.release());
    RF_HIP(p->stats.reserve(2 * cap * sizeof(double)));
  }
  if (p->graphs.count(n)) return 0;
  if (int rc = ensure_x(p)) return rc;
  RF_HIP(hipStreamSynchronize(p->stream));
  rf_plan::BatchGraph bg;
  RF_HIP(hipStreamBeginCapture(p->stream, hipStreamCaptureModeThreadLocal));
  const int rc = batch_issue(p, n);
  hipError_t e2 = hipStreamEndCapture(p->stream, &bg.graph);
  if (rc) return rc;
  RF_HIP(e2);
  RF_HIP(hipGraphInstantiate(&bg.exec, bg.graph, nullptr, nullptr, 0));
  p->graphs[n] = bg;
  return 0;
}

int rf_realise_batch_prepare(rf_plan* p, int n) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  if (!route(p).single()) return 0;     // slab / generic batches are not graph-captured
  return batch_prepare(p, n);
}

int rf_realise_batch(rf_plan* p, const uint64_t* seeds, int n, double* rms_out) {
  RF_REQUIRE(p && seeds, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(n >= 1, "need at least one seed");
  const Route r = route(p);
  if (r.exchanges() || r.replicates()) {
    RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
    RF_HIP(hipSetDevice(p->device));
    if (int rc = slab_batch(p, r, seeds, n)) return rc;
    return rms_out ? rms_from_stats(p, n, rms_out) : 0;
  }
  if (r.kind == Route::Generic) {             // no graph: realisations one after the other
    RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
    RF_HIP(hipSetDevice(p->device));
    if (int rc = ensure_stats(p, n)) return rc;
    const bool fused = p->fused_generic;        // generation inside the x pass: no K, what it holds as it was (queue_c2r)
    if (!fused) { if (int rc = ensure_k(p)) return rc; }
    RF_HIP(p->tl.begin(p->stream, false));
    for (int i = 0; i < n; ++i) {
      const GenParams gp = make_gen(p, seeds[i], RF_NOISE_NATIVE);
      if (!fused) RF_HIP(launch_gen_kspace(p->f64, p->K.ptr, gp, p->stream));
      if (int rc = generic_c2r(p, p->K.ptr, p->stats.get() + 2 * i, nullptr, fused ? &gp : nullptr)) return rc;
    }
    RF_HIP(p->tl.end(p->stream));
    p->has.field_ready(p->W.ptr, n - 1);
    if (!fused) p->has.kspace_ready();
    return rms_out ? rms_from_stats(p, n, rms_out) : 0;
  }
  if (int rc = batch_prepare(p, n)) return rc;
  if (p->seeds_pin[0].bytes < n * sizeof(uint64_t) || p->seeds_pin[1].bytes < n * sizeof(uint64_t)) {
    RF_HIP(hipStreamSynchronize(p->stream));
    for (auto& slot : p->seeds_pin) RF_HIP(slot.reserve((size_t)(n + 64) * sizeof(uint64_t)));
  }
  RF_HIP(p->seeds_ev.ensure(2, hipEventDisableTiming));
  const int slot = p->seeds_turn;
  p->seeds_turn ^= 1;
  RF_HIP(hipEventSynchronize(p->seeds_ev[slot]));        // returns at once for an event that was never recorded
  std::memcpy(p->seeds_pin[slot].get(), seeds, n * sizeof(uint64_t));
  RF_HIP(hipMemcpyAsync(p->seeds_dev.get(), p->seeds_pin[slot].get(), n * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipEventRecord(p->seeds_ev[slot], p->stream));
  RF_HIP(p->tl.begin(p->stream, false));
  RF_HIP(hipGraphLaunch(p->graphs[n].exec, p->stream));
  RF_HIP(p->tl.end(p->stream));
  p->has.field_ready(p->W.ptr, n - 1);
  return rms_out ? rms_from_stats(p, n, rms_out) : 0;
}

int rf_moments(rf_plan* p, double* mean, double* std_out) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->has.moments(), "no realisation has been computed");
  RF_HIP(hipSetDevice(p->device));
  double st[2];
  RF_HIP(hipMemcpyAsync(st, p->stats.get() + 2 * p->has.moments_pair(), sizeof(st), hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  mean_std(p, st, mean, std_out);
  return 0;
}

int rf_lognormal(rf_plan* p, const double* a_z, const double* b_z, int nz, double sigma) {
  RF_REQUIRE(p && a_z && b_z, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(nz == p->nz, "table length must equal nz");
  RF_REQUIRE(p->has.field(), "no real-space field on the device");
  RF_REQUIRE(sigma > 0, "sigma must be positive");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(p->ztab.get(), a_z, nz * sizeof(double), hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipMemcpyAsync(p->ztab.get() + nz, b_z, nz * sizeof(double), hipMemcpyHostToDevice, p->stream));
  RF_HIP(launch_lognormal(p->f64, p->has.where(), (long long)p->nxl * p->ny, nz, p->ztab.get(), p->ztab.get() + nz, sigma, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));  // host tables may go away
  p->has.field_modified();
  return 0;
}

int rf_set_z_tables(rf_plan* p, const double* growth_z, const double* density_z, int nz) {
  RF_REQUIRE(p && growth_z, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(nz == p->nz, "table length must equal nz");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipStreamSynchronize(p->stream));
  RF_HIP(p->lntab.reserve((4 * (size_t)nz + 8) * sizeof(double)));
  RF_HIP(hipMemcpy(p->lntab.get(), growth_z, nz * sizeof(double), hipMemcpyHostToDevice));
  if (density_z) RF_HIP(hipMemcpy(p->lntab.get() + nz, density_z, nz * sizeof(double), hipMemcpyHostToDevice));
  p->ln_tables = true;
  p->ln_density = density_z != nullptr;
  return 0;
}

// rows K,T,R,S + the c2r transform + the lognormal map, with sigma = the field's rms taken from the y pass (Parseval) so that the
// map runs in the z pass's epilogue: generate_delta_field(save_potential=False) followed by convert_delta_to_density()
// (generate.py:191-199,218-219 and 266-273, cosmotools.py:206-221) in 5 sweeps instead of 7 and without the host round trip.
int rf_realise_lognormal(rf_plan* p, uint64_t seed, int mode, const double* noise_host, double* sigma_out) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->have_kgrid && p->have_power, "rf_set_kgrid and rf_set_power must be called first");
  RF_REQUIRE(p->ln_tables, "rf_set_z_tables must be called first");
  RF_REQUIRE(route(p).single(), "rf_realise_lognormal is for single-GPU plans with power-of-two axes");
  RF_REQUIRE(mode == RF_NOISE_NATIVE || mode == RF_NOISE_EXTERNAL || mode == RF_NOISE_RESIDENT, "unknown noise mode");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = upload_noise(p, mode, noise_host)) return rc;
  const CallDesc cd(mode);
  const long long nzl = p->nzl, ntiles = (long long)p->nx * nzl / col_tile_cols(p->f64, p->ny);
  RF_HIP(p->ypart.reserve(ntiles * sizeof(double)));
  hipStream_t s = p->stream;
  const GenParams gp = make_gen(p, seed, mode);
  const ColGeom gy{nzl, (long long)p->ny * nzl, nzl};
  const double n3 = (double)p->nx * (double)p->ny * (double)p->nz, scale = inv_cells(p);
  double *growth = p->lntab.get(), *dens = p->lntab.get() + p->nz, *A = p->lntab.get() + 2 * p->nz, *B = p->lntab.get() + 3 * p->nz, *sig = p->lntab.get() + 4 * p->nz;
  Timeline* tl = &p->tl;
  RF_HIP(tl->begin(s, true));
  // into W, the plain layout whatever RF_FLAG_TRANSPOSED_INTERMEDIATE says: the accumulating y pass runs in place on W
  // (timed: rf_kernel_ms reports x, y + tables, z + map, reduce of this call too)
  if (int rc = queue_x(p, cd, gp, nullptr, p->W.ptr, s, tl)) return rc;
  RF_HIP(mark(tl, rft::X, s));
  RF_HIP(launch_col_plain_acc(p->f64, p->ny, p->W.ptr, gy, (long long)p->nx * nzl, p->kz0, (int)nzl, p->ypart.get(), p->tw_y.ptr, s));
  // rms = sqrt(S / (nx ny)) / N3  (rf_fft.h AccColIO)
  RF_HIP(launch_lognormal_tables(p->ypart.get(), ntiles, 1.0 / ((double)p->nx * (double)p->ny * n3 * n3), growth, p->ln_density ? dens : nullptr, p->nz,
                                 p->f64 ? 0 : 1, p->f64 ? lognormal_ap_unit<double>(scale) : 1.0, sig, A, B, s));
  RF_HIP(mark(tl, rft::Y, s));
  RF_HIP(launch_row_c2r_lognormal(p->f64, (int)p->nzc, p->W.ptr, (long long)p->nx * p->ny, scale, A, B, p->tw_z.ptr, p->partials.get(), s));
  RF_HIP(mark(tl, rft::Z, s));
  RF_HIP(launch_reduce_partials(p->partials.get(), p->npartials, p->stats.get(), p->partials.get() + 2 * p->npartials, s));
  RF_HIP(tl->end(s));
  p->has.field_ready(p->W.ptr, 0);                                 // (the moments of the DENSITY field now)
  p->has.kspace_consumed();
  if (sigma_out) {
    RF_HIP(hipMemcpyAsync(sigma_out, sig, sizeof(double), hipMemcpyDeviceToHost, s));
    RF_HIP(hipStreamSynchronize(s));
  }
  return 0;
}

int rf_affine_z(rf_plan* p, const double* mul_z, int nz, double add) {
  RF_REQUIRE(p && mul_z, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(nz == p->nz, "table length must equal nz");
  RF_REQUIRE(p->has.field(), "no real-space field on the device");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(p->ztab.get(), mul_z, nz * sizeof(double), hipMemcpyHostToDevice, p->stream));
  RF_HIP(launch_affine_z(p->f64, p->has.where(), (long long)p->nxl * p->ny, nz, p->ztab.get(), add, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  p->has.field_modified();
  return 0;
}

int rf_scale_z(rf_plan* p, const double* factor_z, int nz) { return rf_affine_z(p, factor_z, nz, 0.0); }

// Lensing potential psi of the real field on the device (the Newtonian potential on the light cone) into the
// auxiliary buffer: generate.py:352-416 with cot_z = cotK(D) (generate.py:383-395) and D = spacing * iz.
int rf_lensing_potential(rf_plan* p, const double* cot_z, int nz, double spacing, int i_min) {
  RF_REQUIRE(p && cot_z, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(nz == p->nz, "table length must equal nz");
  RF_REQUIRE(i_min >= 0 && i_min < nz, "invalid i_min");
  RF_REQUIRE(spacing > 0, "spacing must be positive");
  RF_REQUIRE(p->has.field(), "no real-space field on the device");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_k(p)) return rc;            // (nx ny (nz/2+1)) complex >= (nx ny nz) real
  RF_HIP(hipMemcpyAsync(p->ztab.get(), cot_z, nz * sizeof(double), hipMemcpyHostToDevice, p->stream));
  RF_HIP(launch_lensing(p->f64, p->has.where(), p->K.ptr, (long long)p->nxl * p->ny, nz, p->ztab.get(), spacing, i_min, p->stream));   // rows are local: x slab
  RF_HIP(hipStreamSynchronize(p->stream));
  p->has.aux_ready();
  return 0;
}

// planes [x0, x1) of the auxiliary real field (dense [nx][ny][nz])
int rf_download_aux(rf_plan* p, void* host, int x0, int x1) {
  RF_REQUIRE(p && host, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->K.ptr && p->has.aux(), "no auxiliary field on the device");
  RF_REQUIRE(0 <= x0 && x0 < x1 && x1 <= p->nxl, "invalid x range (multi-GPU plans hold nx/ranks local planes)");
  RF_HIP(hipSetDevice(p->device));
  const size_t plane = (size_t)p->ny * p->nz * (p->csize / 2);
  RF_HIP(hipMemcpyAsync(host, (const char*)p->K.ptr + (size_t)x0 * plane, (size_t)(x1 - x0) * plane, hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

int rf_save_potential(rf_plan* p) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->K.ptr && p->has.kspace(), "no k-space data");
  RF_REQUIRE(p->have_kgrid, "rf_set_kgrid must be called first");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_p(p)) return rc;
  p->has.potential2_stale();
  RF_HIP(launch_save_potential(p->f64, p->K.ptr, p->P.ptr, p->nx, p->ny, p->nz, p->kx2.get(), p->ky2.get(), p->kz2.get(), p->nzl + 1, p->kz0, p->ppitch, p->stream));
  return 0;
}

int rf_load_potential(rf_plan* p, double scale) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->P.ptr, "no saved potential");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_k(p)) return rc;
  RF_HIP(launch_scale_copy(p->f64, p->P.ptr, p->K.ptr, (long long)p->nx * p->ny * (p->nzl + 1), (int)p->nzl + 1, p->ppitch, scale, p->stream));
  p->has.kspace_ready();
  return 0;
}

}  // extern "C"
namespace rfc {
// What the gradient and the Hessian calls share once each has refused what only it refuses: the source must be there -- the stored
// potential or the second-order one (rows of ppitch cells), or the plan's k-space array in divide mode -- and the fields that both
// parameter structs have (rf_core.h GradParams, HessParams)
template <class P>
int derivative_source(rf_plan* p, int source, P& g, const void*& S) {
  if (source == RF_GRAD_FROM_POTENTIAL) RF_REQUIRE(p->P.ptr, "no saved potential");
  else if (source == RF_GRAD_FROM_POTENTIAL2) RF_REQUIRE(p->L.ptr && p->has.potential2(), "no second-order potential: call rf_lpt2_potential first");
  else {
    RF_REQUIRE(p->K.ptr && p->has.kspace(), "no k-space data: call rf_generate or rf_upload_k first");
    RF_REQUIRE(p->have_kgrid, "rf_set_kgrid must be called first");
  }
  g.nx = p->nx; g.ny = p->ny; g.nz = p->nz;
  g.divide = source == RF_GRAD_FROM_KSPACE;
  g.kx2 = p->kx2.get(); g.ky2 = p->ky2.get(); g.kz2 = p->kz2.get();
  g.pitch = g.divide ? p->nzc + 1 : p->ppitch;
  S = g.divide ? p->K.ptr : (source == RF_GRAD_FROM_POTENTIAL2 ? p->L.ptr : p->P.ptr);
  return 0;
}
int gradient_params(rf_plan* p, int axis, double scale, double dk, int source, GradParams& g, const void*& S) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->nranks == 1, "the gradient of the potential runs on single-rank plans");
  RF_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2");
  RF_REQUIRE(source == RF_GRAD_FROM_POTENTIAL || source == RF_GRAD_FROM_KSPACE || source == RF_GRAD_FROM_POTENTIAL2,
             "source must be RF_GRAD_FROM_POTENTIAL, RF_GRAD_FROM_KSPACE or RF_GRAD_FROM_POTENTIAL2");
  memset(&g, 0, sizeof(g));
  g.axis = axis;
  g.sdk = scale * dk;
  return derivative_source(p, source, g, S);
}
int hessian_params(rf_plan* p, int a, int b, double scale, double dk_a, double dk_b, int source, HessParams& g, const void*& S) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->nranks == 1, "the Hessian of the potential runs on single-rank plans");
  RF_REQUIRE(a >= 0 && a <= 2 && b >= 0 && b <= 2, "axes must be 0, 1 or 2");
  RF_REQUIRE(a <= b, "axes must be given as a <= b");
  RF_REQUIRE(source == RF_GRAD_FROM_POTENTIAL || source == RF_GRAD_FROM_KSPACE, "source must be RF_GRAD_FROM_POTENTIAL or RF_GRAD_FROM_KSPACE");
  memset(&g, 0, sizeof(g));
  g.a = a; g.b = b;
  g.sdk2 = -scale * dk_a * dk_b;
  return derivative_source(p, source, g, S);
}
// K = the component (rf_load_gradient / rf_load_hessian)
template <class P>
int load_derivative(rf_plan* p, const P& g, const void* S) {
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_k(p)) return rc;
  RF_HIP(launch_derivative(p->f64, S, p->K.ptr, g, p->stream));
  p->has.kspace_ready();
  return 0;
}
// the component as a real field (rf_execute_gradient_c2r / rf_execute_hessian_c2r).  RF_GRAD_FROM_KSPACE consumes K on either kind of
// plan: a tiled plan overwrites it, and the generic form, which only reads it, keeps to the same contract.
template <class P>
int execute_derivative_c2r(rf_plan* p, const P& g, const void* S, int source) {
  RF_HIP(hipSetDevice(p->device));
  if (!p->generic) {    // the component as a sweep of its own, then the plan's inverse transform
    if (int rc = load_derivative(p, g, S)) return rc;
    const int rc = rf_execute_c2r(p);
    if (source == RF_GRAD_FROM_KSPACE) p->has.kspace_consumed();
    return rc;
  }
  // generic plans: the factor is applied by the x pass to the cells it loads (rf_generic.h generic_c2r_from_seq); K, P are only read
  RF_HIP(p->tl.begin(p->stream, true));             // (rf_kernel_ms: x with the factor, y, contiguous, reduce; [4] = the sweep of a plan whose x axis is split)
  if (int rc = generic_c2r(p, S, p->stats.get(), &p->tl, &g)) return rc;
  RF_HIP(p->tl.end(p->stream));
  p->has.field_ready(p->W.ptr, 0);
  if (source == RF_GRAD_FROM_KSPACE) p->has.kspace_consumed();
  return 0;
}
// the accumulators of rf_lpt2_source, later the second-order potential
int ensure_l(rf_plan* p) { RF_HIP(p->L.reserve(2 * p->w_bytes > p->p_bytes ? 2 * p->w_bytes : p->p_bytes)); return 0; }
// the particle buffers (rf_particles_*): the displacements, zeroed once, and the paint's accumulator grid with its drop counter
size_t particle_cells(const rf_plan* p) { return (size_t)p->nx * p->ny * p->nz; }
int ensure_q(rf_plan* p) {
  if (p->Q) return 0;
  RF_HIP(p->Q.reserve(3 * p->w_bytes));
  RF_HIP(hipMemsetAsync(p->Q.ptr, 0, 3 * p->w_bytes, p->stream));
  return 0;
}
int ensure_a(rf_plan* p) {
  RF_HIP(p->pa_drop.reserve(8));
  RF_HIP(p->A.reserve(particle_cells(p) * 8));
  return 0;
}
int ensure_pg(rf_plan* p) {
  RF_HIP(p->pa_drop.reserve(8));
  if (p->PG) return 0;
  RF_HIP(p->PG.reserve(3 * p->w_bytes));
  RF_HIP(hipMemsetAsync(p->PG.ptr, 0, 3 * p->w_bytes, p->stream));
  return 0;
}
}  // namespace rfc
extern "C" {

int rf_load_gradient(rf_plan* p, int axis, double scale, double dk, int source) {
  GradParams g;
  const void* S = nullptr;
  if (int rc = gradient_params(p, axis, scale, dk, source, g, S)) return rc;
  return load_derivative(p, g, S);
}

int rf_execute_gradient_c2r(rf_plan* p, int axis, double scale, double dk, int source) {
  GradParams g;
  const void* S = nullptr;
  if (int rc = gradient_params(p, axis, scale, dk, source, g, S)) return rc;
  return execute_derivative_c2r(p, g, S, source);
}

int rf_load_hessian(rf_plan* p, int a, int b, double scale, double dk_a, double dk_b, int source) {
  HessParams g;
  const void* S = nullptr;
  if (int rc = hessian_params(p, a, b, scale, dk_a, dk_b, source, g, S)) return rc;
  return load_derivative(p, g, S);
}

int rf_execute_hessian_c2r(rf_plan* p, int a, int b, double scale, double dk_a, double dk_b, int source) {
  HessParams g;
  const void* S = nullptr;
  if (int rc = hessian_params(p, a, b, scale, dk_a, dk_b, source, g, S)) return rc;
  return execute_derivative_c2r(p, g, S, source);
}

// S(x) = sum_{a<b} (H_aa H_bb - H_ab^2) of the stored potential (rf_core.h lpt2_step): six Hessian transforms with scale 1 in the order
// xx, yy, zz, xy, xz, yz, each followed by its step of the sweep over the field buffer and the accumulators in L
int rf_lpt2_source(rf_plan* p, const double* dk) {
  RF_REQUIRE(p && dk, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->nranks == 1, "the second-order source runs on single-rank plans");
  RF_REQUIRE(p->P.ptr, "no saved potential");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_l(p)) return rc;
  p->has.potential2_stale();                         // (the accumulators take the memory of the second-order potential)
  static const int comp[6][3] = {{0, 0, LPT2_FIRST}, {1, 1, LPT2_DIAG2}, {2, 2, LPT2_DIAG3}, {0, 1, LPT2_OFF}, {0, 2, LPT2_OFF}, {1, 2, LPT2_LAST}};
  void* T = p->L.ptr;
  void* S = (char*)p->L.ptr + p->w_bytes;
  const long long n = (long long)p->nx * p->ny * p->nz;
  for (const auto& c : comp) {
    if (int rc = rf_execute_hessian_c2r(p, c[0], c[1], 1.0, dk[c[0]], dk[c[1]], RF_GRAD_FROM_POTENTIAL)) return rc;
    RF_HIP(launch_lpt2_accumulate(p->f64, c[2], p->W.ptr, T, S, n, p->stream));
  }
  RF_HIP(p->tl.end(p->stream));                      // (rf_elapsed_ms: the last component's transform and the last step ...
  p->tl.detailed = false;                            // ... which no entry of rf_kernel_ms describes: refused, as it always was)
  p->has.field_written(p->W.ptr);
  p->has.kside_cleared();                            // (tiled plans left a Hessian component there: one contract)
  return 0;
}

// phi2(k) = rfftn(S)(k) / k^2 into L, in the stored potential's layout: the source, the forward transform, the division
int rf_lpt2_potential(rf_plan* p, const double* dk) {
  RF_REQUIRE(p && dk, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->nranks == 1, "the second-order potential runs on single-rank plans");
  RF_REQUIRE(p->P.ptr, "no saved potential");
  RF_REQUIRE(p->have_kgrid, "rf_set_kgrid must be called first");
  if (int rc = rf_lpt2_source(p, dk)) return rc;
  if (int rc = rf_execute_r2c(p)) return rc;
  RF_HIP(launch_save_potential(p->f64, p->K.ptr, p->L.ptr, p->nx, p->ny, p->nz, p->kx2.get(), p->ky2.get(), p->kz2.get(), p->nzl + 1, p->kz0, p->ppitch, p->stream));
  RF_HIP(p->tl.end(p->stream));
  p->has.potential2_ready();
  return 0;
}

// ---- particles: the resident displacement buffer and the cloud-in-cell paint (rf_core.h cic_*; rf_k_particles.hip) ----
static int particles_check(rf_plan* p, const char* multi) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->nranks == 1, multi);
  return 0;
}
static int inv_h_check(const double* inv_h) {
  for (int a = 0; a < 3; ++a) RF_REQUIRE(inv_h[a] > 0 && inv_h[a] <= 1.7976931348623157e308, "inv_h must be positive and finite");
  return 0;
}
// component `axis` of the displacements Q, slot `slot` of the gathered values PG
static char* q_component(rf_plan* p, int axis) { return (char*)p->Q.ptr + (size_t)axis * p->w_bytes; }
static char* pg_slot(rf_plan* p, int slot) { return (char*)p->PG.ptr + (size_t)slot * p->w_bytes; }
// one real array between the host and the device, complete on return
static int particles_copy(rf_plan* p, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(dst, src, bytes, kind, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}
// the drop counter around a sweep: cleared on the stream before it; copied out after it, the stream drained
static hipError_t drop_clear(rf_plan* p) { return hipMemsetAsync(p->pa_drop.ptr, 0, 8, p->stream); }
static int drop_read(rf_plan* p, unsigned long long* dropped) { return particles_copy(p, dropped, p->pa_drop.ptr, 8, hipMemcpyDeviceToHost); }

int rf_particles_accumulate(rf_plan* p, int axis, double coeff, int first) {
  if (int rc = particles_check(p, "the particle displacements live on single-rank plans")) return rc;
  RF_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2");
  RF_REQUIRE(p->has.field(), "no real-space field on the device");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_q(p)) return rc;
  RF_HIP(launch_particles_accumulate(p->f64, p->has.where(), q_component(p, axis), coeff, first, (long long)particle_cells(p), p->stream));
  return 0;
}

int rf_particles_upload(rf_plan* p, int axis, const void* host) {
  if (int rc = particles_check(p, "the particle displacements live on single-rank plans")) return rc;
  RF_REQUIRE(host, "null argument");
  RF_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_q(p)) return rc;
  return particles_copy(p, q_component(p, axis), host, p->w_bytes, hipMemcpyHostToDevice);
}

int rf_particles_download(rf_plan* p, int axis, void* host) {
  if (int rc = particles_check(p, "the particle displacements live on single-rank plans")) return rc;
  RF_REQUIRE(host, "null argument");
  RF_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2");
  RF_REQUIRE(p->Q.ptr, "no particle displacements: call rf_particles_accumulate or rf_particles_upload first");
  return particles_copy(p, host, q_component(p, axis), p->w_bytes, hipMemcpyDeviceToHost);
}

// A <- 0, the scatter, W <- (double)A 2^-48 - 1.  rf_kernel_ms afterwards: [0] clearing A, [1] the scatter, [2] the conversion, [3] = [4] = 0
int rf_particles_paint(rf_plan* p, const double* inv_h, unsigned long long* dropped) { return rf_particles_paint_ex(p, inv_h, RF_ASSIGN_CIC, dropped); }

// the same with the assignment scheme as an argument of the call (RF_ASSIGN_CIC, RF_ASSIGN_TSC); any other is refused with nothing queued
int rf_particles_paint_ex(rf_plan* p, const double* inv_h, int scheme, unsigned long long* dropped) {
  return rf_particles_paint_shifted(p, inv_h, scheme, 0, dropped);
}

// what every paint refuses, with nothing queued
static int paint_refuse(rf_plan* p, const double* inv_h, int scheme, int half_cell, const unsigned long long* dropped) {
  if (int rc = particles_check(p, "the cloud-in-cell paint runs on single-rank plans")) return rc;
  RF_REQUIRE(inv_h && dropped, "null argument");
  RF_REQUIRE(scheme == RF_ASSIGN_CIC || scheme == RF_ASSIGN_TSC, "scheme is RF_ASSIGN_CIC (2) or RF_ASSIGN_TSC (3)");
  RF_REQUIRE(half_cell == 0 || half_cell == 1, "half_cell is 0 or 1");
  RF_REQUIRE(p->Q.ptr, "no particle displacements: call rf_particles_accumulate or rf_particles_upload first");
  return inv_h_check(inv_h);
}
static int paint_queue(rf_plan* p, const double* inv_h, int scheme, int half_cell);

// ... and with the half-cell shift of an interlaced paint's second grid (rf_core.h cic_axis_half): half_cell = 0 is rf_particles_paint_ex
int rf_particles_paint_shifted(rf_plan* p, const double* inv_h, int scheme, int half_cell, unsigned long long* dropped) {
  if (int rc = paint_refuse(p, inv_h, scheme, half_cell, dropped)) return rc;
  if (int rc = paint_queue(p, inv_h, scheme, half_cell)) return rc;
  return drop_read(p, dropped);
}
// the paint itself, queued: the arguments were checked, and the drop counter is left on the device for drop_read (a host synchronisation)
static int paint_queue(rf_plan* p, const double* inv_h, int scheme, int half_cell) {
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_a(p)) return rc;
  const size_t n = particle_cells(p);
  // auto: the tiled form, the faster one at 1024^3 and 1000^3 on both displacement scales measured (rms 0.1 and 2 cells: 13 against 208 ms and
  // 64 against 357 ms of scatter; profiles/paint_bench.log)
  // The triangular-shaped cloud: the tiled form too, 16.3 against 185 ms and 254 against 1200 ms of scatter at 1024^3 (15.9 / 167 and
  // 253 / 1108 ms at 1000^3), rms 0.1 and 2 cells, spread between rounds below 10 ms (profiles/tsc_bench.log)
  const int form = p->paint_form ? p->paint_form : 2;
  p->has.counts_stale();
  RF_HIP(p->tl.begin(p->stream, true));
  RF_HIP(hipMemsetAsync(p->A.ptr, 0, n * 8, p->stream));
  RF_HIP(drop_clear(p));
  RF_HIP(p->tl.mark(rft::X, p->stream));
  RF_HIP(launch_cic_paint(p->f64, scheme, form, half_cell, p->Q.ptr, (unsigned long long*)p->A.ptr, (unsigned long long*)p->pa_drop.ptr, p->nx, p->ny, p->nz, inv_h, p->stream));
  RF_HIP(p->tl.mark(rft::Y, p->stream));
  RF_HIP(launch_cic_convert(p->f64, (const unsigned long long*)p->A.ptr, p->W.ptr, (long long)n, p->stream));
  RF_HIP(p->tl.mark(rft::Z, p->stream));
  RF_HIP(p->tl.end(p->stream));
  p->has.field_written(p->W.ptr);
  p->has.counts_ready();
  return 0;
}

// ---- the interlaced paint: a stashed second half spectrum and the combine (rf_core.h interlace_cell; rf_k_misc.hip interlace_kernel) ----
static int kspace_pair_check(rf_plan* p) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->nranks == 1, "the stashed spectrum and the interlacing combine live on single-rank plans");
  return 0;
}
static int ensure_ks(rf_plan* p) { RF_HIP(p->KS.reserve(p->k_bytes)); return 0; }
// the three phase tables (null: all ones): refused unless every entry is finite ...
static int interlace_tables_check(rf_plan* p, const double* const (&tab)[3]) {
  const int len[3] = {p->nx, p->ny, p->nz / 2 + 1};
  for (int a = 0; a < 3; ++a)
    for (int i = 0; tab[a] && i < 2 * len[a]; ++i) RF_REQUIRE(std::isfinite(tab[a][i]), "bad phase table: every entry must be finite");
  return 0;
}
// ... and on the device when this returns, dev[a] the device address of table a or null
static int interlace_tables_upload(rf_plan* p, const double* const (&tab)[3], const double* (&dev)[3]) {
  const int len[3] = {p->nx, p->ny, p->nz / 2 + 1};
  if (!tab[0] && !tab[1] && !tab[2]) { dev[0] = dev[1] = dev[2] = nullptr; return 0; }
  const size_t need = 2 * ((size_t)len[0] + len[1] + len[2]) * sizeof(double);
  if (p->il_tab.bytes < need) RF_HIP(hipStreamSynchronize(p->stream));
  RF_HIP(p->il_tab.reserve(need));
  double* d = p->il_tab.get();
  for (int a = 0; a < 3; ++a) {
    dev[a] = tab[a] ? d : nullptr;
    if (tab[a]) RF_HIP(hipMemcpyAsync(d, tab[a], 2 * (size_t)len[a] * sizeof(double), hipMemcpyHostToDevice, p->stream));
    d += 2 * len[a];
  }
  RF_HIP(hipStreamSynchronize(p->stream));            // (the caller's arrays are its own again)
  return 0;
}

// S <- K
int rf_kspace_stash(rf_plan* p) {
  if (int rc = kspace_pair_check(p)) return rc;
  RF_REQUIRE(p->K.ptr && p->has.kspace(), "no k-space data: call rf_generate or rf_upload_k first");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_ks(p)) return rc;
  RF_HIP(p->tl.begin(p->stream, false));
  RF_HIP(hipMemcpyAsync(p->KS.ptr, p->K.ptr, p->k_bytes, hipMemcpyDeviceToDevice, p->stream));
  RF_HIP(p->tl.end(p->stream));
  p->has.stash_ready();
  return 0;
}

// K <- (S + p K) / 2; the stash stays as it is
int rf_kspace_interlace(rf_plan* p, const double* px, const double* py, const double* pz) {
  if (int rc = kspace_pair_check(p)) return rc;
  RF_REQUIRE(p->KS.ptr && p->has.stash(), "no stashed spectrum: call rf_kspace_stash first");
  RF_REQUIRE(p->K.ptr && p->has.kspace(), "no k-space data: call rf_generate or rf_upload_k first");
  const double* const tab[3] = {px, py, pz};
  if (int rc = interlace_tables_check(p, tab)) return rc;
  RF_HIP(hipSetDevice(p->device));
  const double* dev[3];
  if (int rc = interlace_tables_upload(p, tab, dev)) return rc;
  RF_HIP(p->tl.begin(p->stream, false));
  RF_HIP(launch_interlace(p->f64, p->KS.ptr, p->K.ptr, dev[0], dev[1], dev[2], p->nx, p->ny, p->nz, p->stream));
  RF_HIP(p->tl.end(p->stream));
  return 0;
}

// The whole interlaced paint: paint, forward transform (its spectrum written straight into the stash: no copy sweep), the shifted paint,
// forward transform, combine, inverse transform.  Afterwards K holds the interlaced spectrum, the field is its inverse transform with
// moments, A holds the SHIFTED paint's counts; *dropped is the first paint's count (the second's equals it: the rule is decided on u).
// rf_elapsed_ms covers the whole call; rf_kernel_ms is refused.  Everything is queued without a host synchronisation in between: the
// drop counter is read once, behind the last step -- the second paint cleared and counted it again, to the same value.
static int paint_interlaced_steps(rf_plan* p, const double* inv_h, int scheme, const double* const (&dev)[3]) {
  if (int rc = paint_queue(p, inv_h, scheme, 0)) return rc;
  if (int rc = queue_r2c_single(p, true, p->KS.ptr)) return rc;
  p->has.stash_ready();
  if (int rc = paint_queue(p, inv_h, scheme, 1)) return rc;
  if (int rc = queue_r2c_single(p, true, nullptr)) return rc;
  RF_HIP(launch_interlace(p->f64, p->KS.ptr, p->K.ptr, dev[0], dev[1], dev[2], p->nx, p->ny, p->nz, p->stream));
  return rf_execute_c2r(p);
}
int rf_particles_paint_interlaced(rf_plan* p, const double* inv_h, int scheme, const double* px, const double* py, const double* pz,
                                  unsigned long long* dropped) {
  if (int rc = paint_refuse(p, inv_h, scheme, 0, dropped)) return rc;
  const double* const tab[3] = {px, py, pz};
  if (int rc = interlace_tables_check(p, tab)) return rc;
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_k(p)) return rc;
  if (int rc = ensure_ks(p)) return rc;
  const double* dev[3];
  if (int rc = interlace_tables_upload(p, tab, dev)) return rc;
  RF_HIP(p->tl.span_begin(p->stream));
  if (int rc = paint_interlaced_steps(p, inv_h, scheme, dev)) { p->tl.span_abandon(); return rc; }
  RF_HIP(p->tl.span_end(p->stream));
  return drop_read(p, dropped);
}

int rf_particles_download_counts(rf_plan* p, unsigned long long* host) {
  if (int rc = particles_check(p, "the cloud-in-cell paint runs on single-rank plans")) return rc;
  RF_REQUIRE(host, "null argument");
  RF_REQUIRE(p->A.ptr && p->has.counts(), "no painted counts: call rf_particles_paint first");
  return particles_copy(p, host, p->A.ptr, particle_cells(p) * 8, hipMemcpyDeviceToHost);
}

int rf_particles_paint_geometry(rf_plan* p, int* brick3, int* halo) {
  RF_REQUIRE(p && brick3 && halo, "null argument");
  cic_paint_geometry(brick3, halo);
  return 0;
}

int rf_particles_set_paint_form(rf_plan* p, int form) {
  if (int rc = particles_check(p, "the cloud-in-cell paint runs on single-rank plans")) return rc;
  RF_REQUIRE(form >= 0 && form <= 2, "form is 0 (auto), 1 (global) or 2 (tiled)");
  p->paint_form = form;
  return 0;
}

// G_slot <- the current real field at the particles (rf_core.h cic_gather_value).  rf_kernel_ms afterwards: [0] the gather, the others 0
int rf_particles_gather(rf_plan* p, const double* inv_h, int slot, double coeff, int first, unsigned long long* dropped) {
  return rf_particles_gather_ex(p, inv_h, RF_ASSIGN_CIC, slot, coeff, first, dropped);
}

// the same with the assignment scheme as an argument of the call (rf_core.h tsc_gather_cells for RF_ASSIGN_TSC)
int rf_particles_gather_ex(rf_plan* p, const double* inv_h, int scheme, int slot, double coeff, int first, unsigned long long* dropped) {
  if (int rc = particles_check(p, "the cloud-in-cell gather runs on single-rank plans")) return rc;
  RF_REQUIRE(inv_h && dropped, "null argument");
  RF_REQUIRE(scheme == RF_ASSIGN_CIC || scheme == RF_ASSIGN_TSC, "scheme is RF_ASSIGN_CIC (2) or RF_ASSIGN_TSC (3)");
  RF_REQUIRE(slot >= 0 && slot <= 2, "slot must be 0, 1 or 2");
  if (int rc = inv_h_check(inv_h)) return rc;
  RF_REQUIRE(p->Q.ptr, "no particle displacements: call rf_particles_accumulate or rf_particles_upload first");
  RF_REQUIRE(p->has.field(), "no real-space field on the device");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_pg(p)) return rc;
  // auto: the tiled form.  At 1024^3 / 1000^3 it takes 13.7 / 13.1 ms against the global form's 28.7 / 39.5 ms on displacements of rms 2
  // cells and 11.2 / 11.1 against 10.1 / 10.1 ms on rms 0.1: it loses 1.1 ms where it loses and wins 15 to 26 ms where it wins, and the
  // displacements' scale is not known without a sweep of its own (profiles/gather_bench.log)
  // The triangular-shaped cloud: the tiled form too.  At 1024^3 / 1000^3 it takes 22.4 / 20.2 ms against the global form's 67.5 / 69.7 ms
  // on rms 2 cells and 14.6 / 14.4 against 12.4 / 12.4 ms on rms 0.1 (spread between rounds 0.3 ms there, 2.2 ms at rms 2): it loses
  // 2.0 to 2.2 ms where it loses and wins 45 to 50 ms where it wins (profiles/tsc_bench.log)
  const int form = p->gather_form ? p->gather_form : 2;
  RF_HIP(drop_clear(p));
  RF_HIP(p->tl.begin(p->stream, true));
  RF_HIP(launch_cic_gather(p->f64, scheme, form, p->Q.ptr, p->has.where(), pg_slot(p, slot), coeff, first, (unsigned long long*)p->pa_drop.ptr, p->nx, p->ny, p->nz, inv_h,
                           p->stream));
  RF_HIP(p->tl.mark(rft::X, p->stream));
  RF_HIP(p->tl.end(p->stream));
  return drop_read(p, dropped);
}

int rf_particles_gather_download(rf_plan* p, int slot, void* host) {
  if (int rc = particles_check(p, "the cloud-in-cell gather runs on single-rank plans")) return rc;
  RF_REQUIRE(host, "null argument");
  RF_REQUIRE(slot >= 0 && slot <= 2, "slot must be 0, 1 or 2");
  RF_REQUIRE(p->PG.ptr, "no gathered values: call rf_particles_gather first");
  return particles_copy(p, host, pg_slot(p, slot), p->w_bytes, hipMemcpyDeviceToHost);
}

// Q_axis = fma(coeff, G_slot, Q_axis): the accumulate sweep with the gathered values in the field's place
int rf_particles_shift(rf_plan* p, int axis, int slot, double coeff) {
  if (int rc = particles_check(p, "the particle displacements live on single-rank plans")) return rc;
  RF_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2");
  RF_REQUIRE(slot >= 0 && slot <= 2, "slot must be 0, 1 or 2");
  RF_REQUIRE(p->Q.ptr, "no particle displacements: call rf_particles_accumulate or rf_particles_upload first");
  RF_REQUIRE(p->PG.ptr, "no gathered values: call rf_particles_gather first");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(launch_particles_accumulate(p->f64, pg_slot(p, slot), q_component(p, axis), coeff, 0, (long long)particle_cells(p), p->stream));
  return 0;
}

int rf_particles_set_gather_form(rf_plan* p, int form) {
  if (int rc = particles_check(p, "the cloud-in-cell gather runs on single-rank plans")) return rc;
  RF_REQUIRE(form >= 0 && form <= 2, "form is 0 (auto), 1 (global) or 2 (tiled)");
  p->gather_form = form;
  return 0;
}

}  // extern "C"
namespace rfc {
// What rf_measure_power and rf_measure_multipoles share (P = PowerParams or MultipoleParams; rf_core.h bin_cell).  The refusals come in
// three runs with the estimator's own between them, in the order the calls have always checked: the plan and the source; the arrays and
// the edges; then, in measure_bins, what the source needs.
int bins_refuse_plan(rf_plan* p, int source) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->nranks == 1, "the power spectrum measurement runs on single-rank plans");
  RF_REQUIRE(source == RF_POWER_FROM_KSPACE || source == RF_POWER_FROM_FIELD, "source must be RF_POWER_FROM_KSPACE or RF_POWER_FROM_FIELD");
  return 0;
}
int bins_refuse_args(const double* k_edges, int nbins, const unsigned long long* count, double* const* sums, int ns) {
  bool all = k_edges && count;
  for (int j = 0; j < ns; ++j) all = all && sums[j];
  RF_REQUIRE(all, "null argument");
  RF_REQUIRE(nbins >= 1 && nbins <= 1024, "nbins must be between 1 and 1024");
  RF_REQUIRE(k_edges[0] >= 0.0, "bad k_edges: the first edge must not be negative");
  for (int b = 0; b < nbins; ++b) RF_REQUIRE(k_edges[b] < k_edges[b + 1], "bad k_edges: the edges must be strictly increasing");
  return 0;
}
// The measurement itself.  g arrives cleared but for the estimator's own fields; its geometry is filled here.  buf is the call's lazy
// buffer: [squared edges, 1025 slots][result planes x 1024][tables: nx, ny, nz/2 + 1 slots, only with comp][planes of per-workgroup
// partials].  comp: three host tables (null entries = all ones) uploaded behind the result, their device addresses stored through
// comp_dev -- or null for an estimator without tables.
template <typename P>
int measure_bins(rf_plan* p, int source, const double* k_edges, int nbins, DevBuf<>& buf, P& g, const double* const* comp, const double** const* comp_dev,
                 unsigned long long* count, double* const (&sums)[BinSums<P>::N]) {
  constexpr BinTable T = bin_table<P>();
  RF_REQUIRE(p->have_kgrid, "rf_set_kgrid must be called first");
  if (source == RF_POWER_FROM_KSPACE) RF_REQUIRE(p->K.ptr && p->has.kspace(), "no k-space data: call rf_generate or rf_upload_k first");
  else RF_REQUIRE(p->has.field_in(p->W.ptr), "no real-space field on the device: call rf_upload_real (or a c2r) first");
  RF_HIP(hipSetDevice(p->device));
  const BinLaunch L = bin_launch_shape(T, p->nx, p->ny, p->nz, nbins);
  const long long plane_words = (long long)L.grid * nbins;
  const int clen[3] = {p->nx, p->ny, p->nz / 2 + 1};
  const size_t tab_words = comp ? (size_t)clen[0] + clen[1] + clen[2] : 0, head_words = 1025 + T.planes * 1024 + tab_words;
  const size_t need = (head_words + T.planes * (size_t)plane_words) * 8;
  if (buf.bytes < need) RF_HIP(hipStreamSynchronize(p->stream));
  RF_HIP(buf.reserve(need));
  double* e2_dev = (double*)buf.ptr;
  unsigned long long* out_dev = (unsigned long long*)buf.ptr + 1025;
  double* tab_dev = (double*)buf.ptr + 1025 + T.planes * 1024;
  unsigned long long* part_dev = (unsigned long long*)buf.ptr + head_words;
  std::vector<double> e2((size_t)nbins + 1);
  for (int b = 0; b <= nbins; ++b) e2[b] = k_edges[b] * k_edges[b];
  RF_HIP(hipMemcpyAsync(e2_dev, e2.data(), e2.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
  for (int a = 0; comp && a < 3; ++a) {
    if (comp[a]) {
      RF_HIP(hipMemcpyAsync(tab_dev, comp[a], (size_t)clen[a] * sizeof(double), hipMemcpyHostToDevice, p->stream));
      *comp_dev[a] = tab_dev;
    }
    tab_dev += clen[a];
  }
  RF_HIP(p->tl.begin(p->stream, false));
  if (source == RF_POWER_FROM_FIELD) { if (int rc = queue_r2c_single(p, false, nullptr)) return rc; }     // tiled plans: W packed, no K
  PowerParams& gp = bin_geom(g);
  gp.nx = p->nx; gp.ny = p->ny; gp.nz = p->nz;
  gp.nbins = nbins;
  gp.packed = source == RF_POWER_FROM_FIELD && !p->generic;
  gp.kz_sorted = 1;
  for (size_t i = 1; i < p->h_kz2.size(); ++i) if (!(p->h_kz2[i - 1] <= p->h_kz2[i])) gp.kz_sorted = 0;
  gp.kx2 = p->kx2.get(); gp.ky2 = p->ky2.get(); gp.kz2 = p->kz2.get();
  RF_HIP(launch_bins(p->f64, gp.packed ? p->W.ptr : p->K.ptr, g, e2_dev, part_dev, plane_words, out_dev, p->stream));
  RF_HIP(p->tl.end(p->stream));
  std::vector<unsigned long long> out(T.planes * (size_t)nbins);
  RF_HIP(hipMemcpyAsync(out.data(), out_dev, out.size() * 8, hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  const size_t nb8 = (size_t)nbins * 8;
  memcpy(count, out.data(), nb8);
  for (int j = 0; j < BinSums<P>::N; ++j) memcpy(sums[j], out.data() + (j + 1) * (size_t)nbins, nb8);
  return 0;
}
}  // namespace rfc
extern "C" {

int rf_measure_power(rf_plan* p, int source, const double* k_edges, int nbins, unsigned long long* count, double* sum_k, double* sum_p) {
  double* const sums[2] = {sum_k, sum_p};
  if (int rc = bins_refuse_plan(p, source)) return rc;
  if (int rc = bins_refuse_args(k_edges, nbins, count, sums, 2)) return rc;
  PowerParams g;
  memset(&g, 0, sizeof(g));
  return measure_bins(p, source, k_edges, nbins, p->pw_buf, g, nullptr, nullptr, count, sums);
}

int rf_measure_multipoles(rf_plan* p, int source, int los_axis, const double* k_edges, int nbins, const double* comp_x, const double* comp_y,
                          const double* comp_z, unsigned long long* count, double* sum_k, double* m0, double* m2, double* m4) {
  double* const sums[4] = {sum_k, m0, m2, m4};
  if (int rc = bins_refuse_plan(p, source)) return rc;
  RF_REQUIRE(los_axis >= 0 && los_axis <= 2, "los_axis must be 0, 1 or 2");
  if (int rc = bins_refuse_args(k_edges, nbins, count, sums, 4)) return rc;
  const double* comp[3] = {comp_x, comp_y, comp_z};
  const int clen[3] = {p->nx, p->ny, p->nz / 2 + 1};
  for (int a = 0; a < 3; ++a)
    for (int i = 0; comp[a] && i < clen[a]; ++i)
      RF_REQUIRE(std::isfinite(comp[a][i]) && comp[a][i] > 0.0, "bad compensation table: every entry must be finite and positive");
  MultipoleParams g;
  memset(&g, 0, sizeof(g));
  g.los = los_axis;
  const double** const comp_dev[3] = {&g.cx, &g.cy, &g.cz};
  return measure_bins(p, source, k_edges, nbins, p->mp_buf, g, comp, comp_dev, count, sums);
}

// ---- the binned bispectrum (rf_core.h shell_cell / bispectrum_add; rf_k_bispectrum.hip) ----
static int bispectrum_check(rf_plan* p) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->nranks == 1, "the bispectrum measurement runs on single-rank plans");
  return 0;
}
// the 8-byte words of bs_part in front of the partials: [squared edges][result][packed triples][amplitude tables]
static size_t bispectrum_head_words(const rf_plan* p) {
  return (BISPECTRUM_MAX_BINS + 1) + BISPECTRUM_MAX_TRIPLES + BISPECTRUM_MAX_TRIPLES / 2 + ((size_t)p->nx + p->ny + p->nz / 2 + 1);
}
// the inverse transform of the masked half spectrum M into the dense real array D, an intermediate of the call: no moments, no host sink
static int bispectrum_c2r(rf_plan* p, const void* M, void* D) {
  if (p->generic) return generic_c2r<GenParams>(p, M, nullptr, nullptr, nullptr, D);
  CallDesc cd;
  cd.intermediate = true;
  return queue_xyz(p, cd, make_gen(p, 0, RF_NOISE_NATIVE), M, D, p->stream, nullptr, nullptr);
}
// For every shell b: filter K into the masked spectrum, transform that into shell field b; then all triples in one reduction.
// rf_kernel_ms afterwards: [0] the shell filters, [1] the transforms, [2] the reduction, the others 0.
int rf_measure_bispectrum(rf_plan* p, const double* k_edges, int nbins, const int* triples, int ntriples, const double* amp_x, const double* amp_y,
                          const double* amp_z, int unit, double* sum3) {
  if (int rc = bispectrum_check(p)) return rc;
  RF_REQUIRE(k_edges && triples && sum3, "null argument");
  RF_REQUIRE(nbins >= 1 && nbins <= BISPECTRUM_MAX_BINS, "nbins must be between 1 and 32");
  RF_REQUIRE(ntriples >= 1 && ntriples <= BISPECTRUM_MAX_TRIPLES, "ntriples must be between 1 and 8192");
  RF_REQUIRE(k_edges[0] >= 0.0, "bad k_edges: the first edge must not be negative");
  for (int b = 0; b < nbins; ++b) RF_REQUIRE(k_edges[b] < k_edges[b + 1], "bad k_edges: the edges must be strictly increasing");
  for (int t = 0; t < ntriples; ++t)
    RF_REQUIRE(0 <= triples[3 * t] && triples[3 * t] <= triples[3 * t + 1] && triples[3 * t + 1] <= triples[3 * t + 2] && triples[3 * t + 2] < nbins,
               "bad triple: every triple must satisfy 0 <= b1 <= b2 <= b3 < nbins");
  const double* amp[3] = {amp_x, amp_y, amp_z};
  const int alen[3] = {p->nx, p->ny, p->nz / 2 + 1};
  for (int a = 0; a < 3 && !unit; ++a)
    for (int i = 0; amp[a] && i < alen[a]; ++i)
      RF_REQUIRE(std::isfinite(amp[a][i]) && amp[a][i] > 0.0, "bad amplitude table: every entry must be finite and positive");
  RF_REQUIRE(p->have_kgrid, "rf_set_kgrid must be called first");
  RF_REQUIRE(p->K.ptr && p->has.kspace(), "no k-space data: call rf_generate or rf_upload_k first");
  const Route r = route(p);
  RF_REQUIRE(r.kind == Route::Generic || r.kind == Route::Single, "the bispectrum measurement runs on the single-GPU pipelines: not with RF_FLAG_FORCE_SLAB_PATH");
  RF_HIP(hipSetDevice(p->device));
  const long long ncells = (long long)p->nx * p->ny * p->nz;
  const BispectrumLaunch L = bispectrum_launch_shape(p->f64, ncells, nbins, ntriples, p->bs_max_wg);
  const size_t head_words = bispectrum_head_words(p), part_bytes = (head_words + (size_t)L.rows * ntriples) * 8, field_bytes = (size_t)nbins * p->w_bytes;
  if (p->bs_mask.bytes < p->k_bytes || p->bs_fields.bytes < field_bytes || p->bs_part.bytes < part_bytes) RF_HIP(hipStreamSynchronize(p->stream));
  p->bs_nbins = 0;                                  // (no shell fields until the call has run to its end)
  RF_HIP(p->bs_mask.reserve(p->k_bytes));
  RF_HIP(p->bs_fields.reserve(field_bytes));
  RF_HIP(p->bs_part.reserve(part_bytes));
  double* e2_dev = (double*)p->bs_part.ptr;
  double* out_dev = e2_dev + (BISPECTRUM_MAX_BINS + 1);
  unsigned* tri_dev = (unsigned*)(out_dev + BISPECTRUM_MAX_TRIPLES);
  double* tab_dev = out_dev + BISPECTRUM_MAX_TRIPLES + BISPECTRUM_MAX_TRIPLES / 2;
  double* part_dev = e2_dev + head_words;
  std::vector<double> e2((size_t)nbins + 1);
  for (int b = 0; b <= nbins; ++b) e2[b] = k_edges[b] * k_edges[b];
  std::vector<unsigned> packed((size_t)ntriples);
  for (int t = 0; t < ntriples; ++t) packed[t] = bispectrum_pack(triples[3 * t], triples[3 * t + 1], triples[3 * t + 2]);
  RF_HIP(hipMemcpyAsync(e2_dev, e2.data(), e2.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipMemcpyAsync(tri_dev, packed.data(), packed.size() * sizeof(unsigned), hipMemcpyHostToDevice, p->stream));
  ShellParams g;
  memset(&g, 0, sizeof(g));
  g.unit = unit != 0;
  const double** const amp_dev[3] = {&g.ax, &g.ay, &g.az};
  for (int a = 0; a < 3; ++a) {
    if (amp[a] && !unit) {
      RF_HIP(hipMemcpyAsync(tab_dev, amp[a], (size_t)alen[a] * sizeof(double), hipMemcpyHostToDevice, p->stream));
      *amp_dev[a] = tab_dev;
    }
    tab_dev += alen[a];
  }
  g.p.nx = p->nx; g.p.ny = p->ny; g.p.nz = p->nz;
  g.p.nbins = nbins;
  g.p.kx2 = p->kx2.get(); g.p.ky2 = p->ky2.get(); g.p.kz2 = p->kz2.get();
  RF_HIP(p->tl.begin(p->stream, true));
  for (int b = 0; b < nbins; ++b) {
    RF_HIP(launch_shell_filter(p->f64, p->K.ptr, p->bs_mask.ptr, g, e2_dev, b, p->bs_max_wg, p->stream));
    RF_HIP(p->tl.mark(rft::X, p->stream));
    if (int rc = bispectrum_c2r(p, p->bs_mask.ptr, (char*)p->bs_fields.ptr + (size_t)b * p->w_bytes)) return rc;
    RF_HIP(p->tl.mark(rft::Y, p->stream));
  }
  RF_HIP(launch_bispectrum_sums(p->f64, p->bs_fields.ptr, ncells, nbins, tri_dev, ntriples, p->bs_max_wg, part_dev, out_dev, p->stream));
  RF_HIP(p->tl.mark(rft::Z, p->stream));
  RF_HIP(p->tl.end(p->stream));
  p->has.field_consumed();                          // the field buffer is the transforms' workspace, on every kind of plan
  RF_HIP(hipMemcpyAsync(sum3, out_dev, (size_t)ntriples * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  p->bs_nbins = nbins;
  return 0;
}

int rf_bispectrum_release(rf_plan* p) {
  if (int rc = bispectrum_check(p)) return rc;
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipStreamSynchronize(p->stream));
  p->bs_nbins = 0;
  RF_HIP(p->bs_mask.release()); RF_HIP(p->bs_fields.release()); RF_HIP(p->bs_part.release());
  return 0;
}

int rf_bispectrum_download_shell(rf_plan* p, int b, void* host) {
  if (int rc = bispectrum_check(p)) return rc;
  RF_REQUIRE(host, "null argument");
  RF_REQUIRE(p->bs_nbins > 0 && p->bs_fields.ptr, "no shell fields: call rf_measure_bispectrum first");
  RF_REQUIRE(b >= 0 && b < p->bs_nbins, "the shell must be one of the last call's bins");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(host, (const char*)p->bs_fields.ptr + (size_t)b * p->w_bytes, p->w_bytes, hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

int rf_bispectrum_geometry(rf_plan* p, int nbins, int ntriples, int* chunk_cells, int* workgroups, int* partial_rows) {
  if (int rc = bispectrum_check(p)) return rc;
  RF_REQUIRE(chunk_cells && workgroups && partial_rows, "null argument");
  RF_REQUIRE(nbins >= 1 && nbins <= BISPECTRUM_MAX_BINS, "nbins must be between 1 and 32");
  RF_REQUIRE(ntriples >= 1 && ntriples <= BISPECTRUM_MAX_TRIPLES, "ntriples must be between 1 and 8192");
  const BispectrumLaunch L = bispectrum_launch_shape(p->f64, (long long)p->nx * p->ny * p->nz, nbins, ntriples, p->bs_max_wg);
  *chunk_cells = L.chunk; *workgroups = (int)L.gx; *partial_rows = L.rows;
  return 0;
}

int rf_bispectrum_set_max_workgroups(rf_plan* p, int n) {
  if (int rc = bispectrum_check(p)) return rc;
  RF_REQUIRE(n >= 0 && n <= 65535, "the workgroup cap is 0 (the default) or between 1 and 65535");
  p->bs_max_wg = n;
  return 0;
}

int rf_upload_k(rf_plan* p, const void* host) {
  RF_REQUIRE(p && host, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_HIP(hipSetDevice(p->device));
  if (int rc = ensure_k(p)) return rc;
  RF_HIP(hipMemcpyAsync(p->K.ptr, host, p->k_bytes, hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  p->has.kspace_ready();
  return 0;
}

int rf_download_k(rf_plan* p, void* host) {
  RF_REQUIRE(p && host, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->K.ptr && p->has.kspace(), "no k-space data");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipMemcpyAsync(host, p->K.ptr, p->k_bytes, hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

int rf_upload_real(rf_plan* p, const void* host, int layout) {
  RF_REQUIRE(p && host, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(!route(p).replicates(), "replicated-generation plans keep no exchange buffers");
  RF_HIP(hipSetDevice(p->device));
  const size_t rsize = p->csize / 2;
  const size_t width = (size_t)p->nz * rsize;
  const size_t hpitch = layout == RF_LAYOUT_PADDED ? (size_t)(p->nz + 2) * rsize : width;
  // (a multi-rank plan takes its own nx / ranks planes)
  RF_HIP(hipMemcpy2DAsync(p->W.ptr, width, host, hpitch, width, (size_t)p->nxl * p->ny, hipMemcpyHostToDevice, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  p->has.field_written(p->W.ptr);
  return 0;
}

int rf_download_real(rf_plan* p, void* host, int layout, int x0, int x1) {
  RF_REQUIRE(p && host, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->has.field(), "no real-space field on the device");
  RF_REQUIRE(0 <= x0 && x0 < x1 && x1 <= p->nxl, "invalid x range (multi-GPU plans hold nx/ranks local planes)");
  RF_HIP(hipSetDevice(p->device));
  const size_t rsize = p->csize / 2;
  const size_t width = (size_t)p->nz * rsize;
  const size_t hpitch = layout == RF_LAYOUT_PADDED ? (size_t)(p->nz + 2) * rsize : width;
  const char* src = (const char*)p->has.where() + (size_t)x0 * p->ny * width;
  RF_HIP(hipMemcpy2DAsync(host, hpitch, src, width, width, (size_t)(x1 - x0) * p->ny, hipMemcpyDeviceToHost, p->stream));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

// generate.py:184-189,230: the reference's calls RETURN a host array, and at 1024^3 the device -> host copy (75 ms over PCIe) is 15 x the
// realisation.  Armed with a host buffer, the NEXT realisation of a single-GPU plan (rf_realise, rf_realise_potential,
// rf_realise_batch_reference ...: everything whose y / z passes run slab by slab on the plan's stream) copies every slab of x planes to
// the host as soon as its z pass has finished, while the GPU runs the following slabs, and returns when the whole field is in `host`
// (layout as rf_download_real): the copy starts ~1.5 ms into a 1024^3 realisation instead of after it.  Ordinary pageable memory.
// One shot: rf_host_sink_delivered says whether the armed call delivered (then rf_download_real is not needed) and disarms.
// host = NULL disarms.
int rf_set_host_sink(rf_plan* p, void* host, int layout) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(route(p).single(), "a host sink serves single-GPU packed plans on the tiled kernels");
  RF_REQUIRE(layout == RF_LAYOUT_DENSE || layout == RF_LAYOUT_PADDED, "invalid layout");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipStreamSynchronize(p->stream));
  p->sink_delivered = false;
  if (p->f64 && (p->sink_host == nullptr) != (host == nullptr)) drop_graphs(p);      // (a float64 plan runs its y / z passes slab by slab only for a sink)
  p->sink_host = host;
  p->sink_layout = layout;
  if (host) RF_HIP(p->dl_stream.create(hipStreamNonBlocking));
  return 0;
}

int rf_host_sink_delivered(rf_plan* p, int* delivered) {
  RF_REQUIRE(p && delivered, "null argument");
  *delivered = p->sink_delivered ? 1 : 0;
  if (p->sink_host && p->f64) { RF_HIP(hipStreamSynchronize(p->stream)); drop_graphs(p); }
  p->sink_host = nullptr;
  p->sink_delivered = false;
  return 0;
}

int rf_device_ptr(rf_plan* p, void** real_field, void** kspace) {
  RF_REQUIRE(p, "null plan");
  if (real_field) *real_field = p->has.where() ? p->has.where() : p->W.ptr;
  if (kspace) *kspace = p->K.ptr;
  return 0;
}

int rf_sync(rf_plan* p) {
  RF_REQUIRE(p, "null plan");
  RF_HIP(hipSetDevice(p->device));
  RF_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

// (the three read-outs refuse before any call and after a call that failed half way: rf_timing.h)
int rf_elapsed_ms(rf_plan* p, float* ms) {
  RF_REQUIRE(p && ms, "null argument");
  RF_REQUIRE(p->tl.complete, "no call of this plan has run to its end: nothing was timed");
  RF_HIP(p->tl.elapsed(ms));
  return 0;
}

// ([4]: the x pass of the fast generation is two launches, the few tiles that hold slot kz = 0 -- with the Hermitian repair -- first; they are
// reported separately so that [0] is the main kernel alone)
int rf_kernel_ms(rf_plan* p, float* ms5) {
  RF_REQUIRE(p && ms5, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  RF_REQUIRE(p->tl.complete && p->tl.detailed, "per-kernel times are recorded by rf_realise / rf_execute_c2r only");
  RF_HIP(p->tl.report(ms5));
  return 0;
}

// 0: one launch per pass and slab always; 1 (default): untimed calls (graph-captured batches, rf_realise_batch_reference) put the z pass
// of slab s and the y pass of slab s + 1 into one launch where rf_k_yz.hip serves the shape; 2: timed calls (rf_realise ...) too
int rf_set_merged_yz(rf_plan* p, int mode) {
  RF_REQUIRE(p, "null plan");
  RF_REQUIRE(mode >= 0 && mode <= 2, "mode is 0, 1 or 2");
  if (p->yz_merge != mode) {
    RF_HIP(hipSetDevice(p->device));
    RF_HIP(hipStreamSynchronize(p->stream));
    drop_graphs(p);                          // (captured batches carry their launches)
    p->yz_merge = mode;
  }
  return 0;
}

// the merged launches of the last timed call under rf_set_merged_yz(2): their summed duration (HIP events on the plan's stream) and number
int rf_merged_yz_ms(rf_plan* p, float* sum_ms, int* launches) {
  RF_REQUIRE(p && sum_ms && launches, "null argument");
  float sum = 0;
  int n = 0;
  if (p->tl.complete && p->tl.detailed) RF_HIP(p->tl.merged(&sum, &n));
  RF_REQUIRE(n > 0, "the last call was not a timed call with merged y / z launches (rf_set_merged_yz(2), a shape rf_k_yz.hip serves)");
  *sum_ms = sum;
  *launches = n;
  return 0;
}

int rf_yz_slabs(rf_plan* p, int* nslab, int* planes) {
  RF_REQUIRE(p && nslab && planes, "null argument");
  RF_REQUIRE(!p->unpacked, "this call does not apply to an unpacked c2c plan");
  const YzSlabs sl = yz_slabs(p->nx, yz_slab_planes(p), p->X.ptr && xpose_ok(p), xpose_row_block(p));
  *planes = sl.count > 1 ? sl.planes : p->nxl;
  *nslab = sl.count;
  return 0;
}

}  // extern "C"
