// rf_emu.cpp -- CPU emulator of the HIP kernels (TEST TOOLING, build container).
//
// Runs the exact phase functions of rf_fft.h / rf_core.h that the gfx950
// kernels inline, one "thread" after another with a plain array standing in
// for LDS and a loop boundary standing in for each workgroup barrier.  It
// checks index math, twiddles, Hermitian packing and the generation rules
// against the oracle without a GPU.  Which configuration a pass takes, which
// launches it makes and how its IO object is filled come from the functions the
// launchers call: rf_select.h and the builders next to each IO type.  It is
// not a product path: nothing in randomfield_amd/ loads it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <pthread.h>
#include <thread>
#include <vector>
#include "../rf_select.h"
#include "../rf_host.h"
#include "../rf_generic.h"

using namespace rf;

namespace {

// The tiles (tile pairs) of one launch: b * mul + add for b in [0, count), less the skipped ones -- a FastStep (rf_select.h), walked with
// fast_step_tile as the kernels walk it.  every(n): the launch over all n tiles.
inline FastStep every(long long n) { return FastStep{FAST_COL, FAST_IO_REPAIR, n, 1, 0, 0, false}; }
// what the last emulated fast generation pass ran (emu_fast_steps): its steps, and how often each tile of the pass was transformed
std::vector<FastStep> g_fast_steps;
std::vector<int> g_fast_visits;
bool g_count_visits = false;
inline void visit(long long tile) { if (g_count_visits && tile >= 0 && tile < (long long)g_fast_visits.size()) ++g_fast_visits[(size_t)tile]; }
struct NoHook { template <class IO> void operator()(long long, const std::vector<IO>&) const {} };

// hook(tile, ios): called after every tile with the threads' IO objects (what the kernel's epilogue reads: AccColIO's sums)
template <class C, int DIR, class IO, class Hook = NoHook>
void run_col_pass(const IO& io_in, const FastStep& run, const cplx<typename C::T>* tw, Hook hook = Hook()) {
  using F = ColFFT<C, DIR, IO>;
  using cx = cplx<typename C::T>;
  std::vector<cx> lds((size_t)(C::LDS_BYTES + IO::LDS_EXTRA) / sizeof(cx));   // exactly the kernel's dynamic LDS
  std::vector<typename F::Regs> regs(C::NT);
  for (long long b = 0; b < run.count; ++b) {
    std::vector<IO> ios(C::NT, io_in);           // every "thread" of a workgroup has its own copy of the kernel argument
    for (auto& io : ios) io.bind_seed();
    const long long tile = io_in.remap_tile(fast_step_tile(run, b));
    visit(tile);
    const cx* ltw = tw;
    if (F::HAS_PROLOGUE) {
      for (int t = 0; t < C::NT; ++t) F::prologue(t, ios[t], tw, lds.data());
      if (C::NPASS >= 2) ltw = F::lds_tw(lds.data());
    }
    for (int t = 0; t < C::NT; ++t) F::pass_first(t, tile, ios[t], lds.data());
    if (C::NPASS == 3) {
      for (int t = 0; t < C::NT; ++t) F::pass_mid_read(t, ltw, lds.data(), regs[t]);
      for (int t = 0; t < C::NT; ++t) F::pass_mid_write(t, lds.data(), regs[t]);
    }
    if (C::NPASS >= 2)
      for (int t = 0; t < C::NT; ++t) F::pass_last(t, tile, ios[t], ltw, lds.data());
    hook(tile, ios);
  }
}

// a pass of length 2 C1::N through Col2 (col2_kernel's phases, a loop boundary for each of its barriers); tw2 = the 2 C1::N-point table
template <class C1, int DIR, class IO>
void run_col2_pass(const IO& io_in, const FastStep& run, const cplx<typename C1::T>* tw2) {
  using X = Col2<C1, DIR, IO>;
  using F = typename X::F;
  using cx = cplx<typename C1::T>;
  std::vector<cx> lds((size_t)(C1::LDS_BYTES + IO::LDS_EXTRA) / sizeof(cx));
  std::vector<typename F::Regs> regs(C1::NT);
  std::vector<typename F::TwRegs> twr(C1::NT);
  std::vector<typename X::Park> pk(C1::NT);
  std::vector<IO> ios(C1::NT, io_in);
  for (auto& io : ios) io.bind_seed();
  for (long long b = 0; b < run.count; ++b) {
    const long long tile = fast_step_tile(run, b);
    visit(tile);
    if (IO::LDS_EXTRA > 0) for (int t = 0; t < C1::NT; ++t) ios[t].prologue(t, C1::NT, F::lds_io(lds.data()));
    for (int t = 0; t < C1::NT; ++t) X::tw_fetch(t, tw2, twr[t]);
    const cx* ltw = F::lds_tw(lds.data());
    for (int phase = 0; phase < 2; ++phase) {
      for (int t = 0; t < C1::NT; ++t) ios[t].set_phase(phase);
      for (int t = 0; t < C1::NT; ++t) F::pass_first(t, tile, ios[t], lds.data());
      if (phase == 0) for (int t = 0; t < C1::NT; ++t) F::tw_stage(t, lds.data(), twr[t]);
      if (C1::NPASS == 3) {
        for (int t = 0; t < C1::NT; ++t) F::pass_mid_read(t, ltw, lds.data(), regs[t]);
        for (int t = 0; t < C1::NT; ++t) F::pass_mid_write(t, lds.data(), regs[t]);
      }
      if (phase == 0) for (int t = 0; t < C1::NT; ++t) X::last_park(t, ltw, lds.data(), pk[t]);
      else for (int t = 0; t < C1::NT; ++t) X::last_combine(t, tile, ios[t], ltw, tw2, lds.data(), pk[t]);
    }
  }
}
// tile pairs with whole-line stores (rf_kernels.h colpair_body, rf_fft_col.h ColPair): phase 0 transforms tile 2p and PARKS the last
// pass's outputs, phase 1 transforms tile 2p + 1 (built without the kz = 0 repair: FIXOK = false) and stores both tiles row by row
template <class C, int DIR, class IO>
void run_colpair_pass(const IO& io_in, const FastStep& run, const cplx<typename C::T>* tw) {
  using X = ColPair<C, DIR, IO>;
  using F = typename X::F;
  using cx = cplx<typename C::T>;
  std::vector<cx> lds((size_t)(C::LDS_BYTES + IO::LDS_EXTRA) / sizeof(cx));
  std::vector<typename F::Regs> regs(C::NT);
  std::vector<typename F::TwRegs> twr(C::NT);
  std::vector<typename F::PreRegs> pre(C::NT);
  std::vector<typename X::Park> pk(C::NT);
  std::vector<IO> ios(C::NT, io_in);
  for (auto& io : ios) io.bind_seed();
  for (long long b = 0; b < run.count; ++b) {
    const long long pair = fast_step_tile(run, b);
    if (IO::LDS_EXTRA > 0) for (int t = 0; t < C::NT; ++t) ios[t].prologue(t, C::NT, F::lds_io(lds.data()));
    for (int t = 0; t < C::NT; ++t) F::tw_fetch(t, tw, twr[t]);
    const cx* ltw = F::lds_tw(lds.data());
    for (int phase = 0; phase < 2; ++phase) {
      const long long tile = 2 * pair + phase;
      visit(tile);
      if (F::PRELOAD) for (int t = 0; t < C::NT; ++t) F::preload(t, tile, ios[t], pre[t]);
      for (int t = 0; t < C::NT; ++t) {
        if (phase == 0) F::template pass_first<true>(t, tile, ios[t], lds.data(), pre[t], F::PRELOAD);
        else F::template pass_first<false>(t, tile, ios[t], lds.data(), pre[t], F::PRELOAD);
      }
      if (phase == 0) for (int t = 0; t < C::NT; ++t) F::tw_stage(t, lds.data(), twr[t]);
      if (C::NPASS == 3) {
        for (int t = 0; t < C::NT; ++t) F::pass_mid_read(t, ltw, lds.data(), regs[t]);
        for (int t = 0; t < C::NT; ++t) F::pass_mid_write(t, lds.data(), regs[t]);
      }
      if (phase == 0) for (int t = 0; t < C::NT; ++t) X::last_park(t, ltw, lds.data(), pk[t]);
      else for (int t = 0; t < C::NT; ++t) X::last_store(t, 2 * pair, ios[t], ltw, lds.data(), pk[t]);
    }
  }
}

// one whole-column pass of length N over all its tiles, on the configuration SEL<T, N> (ColSel, or GenSel for the generating x pass)
template <typename T, int DIR, class IO, template <typename, int> class SEL = ColSel, class Hook = NoHook>
int dispatch_col(int N, const IO& io, long long ncols, Hook hook = Hook()) {
  auto tw = make_twiddles<T>(N);
  return for_col_size(N, -1, [&](auto n) {
    using C = typename SEL<T, decltype(n)::value>::type;
    if (ncols % C::TC) return -2;
    run_col_pass<C, DIR, IO>(io, every(ncols / C::TC), tw.data(), hook);
    return 0;
  });
}

// The in-place strided pass as launch_col_plain (rf_k_col_plain.hip) runs it: two half-length transforms per tile where rf_select.h
// for_col_halves says so and the geometry fits, else the whole column.  emu_set_col_halves(0) keeps the whole column everywhere.
int g_col_halves = 1;
template <typename T, int DIR>
int plain_col_pass(int N, cplx<T>* base, const ColGeom& g, long long ncols) {
  int rc = 0;
  if (g_col_halves && for_col_halves(sizeof(T) == 8, N, g, [&](auto c) {
        using C1 = typename decltype(c)::type;
        if (ncols % C1::TC) { rc = -2; return; }
        auto tw2 = make_twiddles<float>(N);
        run_col2_pass<C1, DIR>(pair2_col_io<Pair2ColIO<float>>((cplx<float>*)base, g), every(ncols / C1::TC), tw2.data());
      }))
    return rc;
  PlainColIO<T> io; io.base = base; io.g = g;
  return dispatch_col<T, DIR>(N, io, ncols);
}
inline ColGeom x_geom(long long ny, long long nzl) { return ColGeom{ny * nzl, 0, ny * nzl}; }       // x pass: C = iy * nzl + kz, row = ix
inline ColGeom y_geom(long long ny, long long nzl) { return ColGeom{nzl, ny * nzl, nzl}; }          // y pass: C = ix * nzl + kz, row = iy

// The hand-off of the x pass's output through the blocked intermediate X [x block][kz tile][ny][rb][tc] (rf_capi.hip queue_xyz /
// queue_yz): y pass in place on X, z pass gathering X -> W.  g_xposed mirrors RF_FLAG_TRANSPOSED_INTERMEDIATE, g_rowblock the rows of
// x per block the plan asks for; whether the shape allows it: rf_select.h xpose_shape_ok.
int g_xposed = 0;          // (RF_FLAG_TRANSPOSED_INTERMEDIATE is off by default)
int g_rowblock = 64;
template <typename T> bool xposed(int nx, int ny, long long nzc) {
  constexpr int f64 = sizeof(T) == 8;
  return g_xposed && xpose_shape_ok(f64, nx, ny, nzc, nzc, col_gen_row_block(f64, nx, g_rowblock));
}
template <typename T> ColGeom xposed_x_geom(int nx, int ny, long long nzl) {
  constexpr int f64 = sizeof(T) == 8;
  return xblock_x_geom(nx, ny, nzl, col_gen_tile_cols(f64, nx), col_gen_row_block(f64, nx, g_rowblock));
}

template <class C, class IO>
void run_row_c2r(const IO& io_in, long long nrows, const cplx<typename C::T>* tw, double* s1, double* s2) {
  using F = RowC2R<C, IO>;
  IO io = io_in;
  using cx = cplx<typename C::T>;
  std::vector<cx> lds((size_t)C::LDS_BYTES / sizeof(cx));
  std::vector<typename F::Regs> regs(C::NT);
  const long long ntiles = (nrows + C::NRT - 1) / C::NRT;
  double a1 = 0, a2 = 0;
  for (long long tile = 0; tile < ntiles; ++tile) {
    for (int t = 0; t < C::NT; ++t) F::prologue(t, tw, lds.data());
    if constexpr (row_io_wants_stage<IO>::value)           // (as row_c2r_kernel: the IO's table into the tile's spare slots, once per tile)
      for (int t = 0; t < C::NT; ++t) io.template stage<C>(t, lds.data());
    const cx* ltw = F::lds_tw(lds.data());
    for (int t = 0; t < C::NT; ++t) F::pass_first(t, tile, nrows, io, ltw, lds.data(), regs[t]);
    if (C::NPASS == 3) {
      for (int t = 0; t < C::NT; ++t) F::pass_mid_read(t, ltw, lds.data(), regs[t]);
      for (int t = 0; t < C::NT; ++t) F::pass_mid_write(t, lds.data(), regs[t]);
    }
    if (C::NPASS >= 2)
      for (int t = 0; t < C::NT; ++t) F::pass_last(t, tile, nrows, io, ltw, lds.data(), regs[t]);
    for (int t = 0; t < C::NT; ++t) { a1 += regs[t].mom.sum(); a2 += regs[t].mom.sumsq(); }
  }
  *s1 = a1; *s2 = a2;
}
// the z pass of rows of M complex with the IO that make_io(Cfg<row configuration>) returns
template <typename T, class MakeIO>
int dispatch_row_c2r(int M, long long nrows, double* s1, double* s2, MakeIO make_io) {
  auto tw = make_twiddles<T>(2 * M);
  return for_row_size(M, -1, [&](auto m) {
    using C = typename RowSel<T, decltype(m)::value>::type;
    auto io = make_io(Cfg<C>{});
    run_row_c2r<C, decltype(io)>(io, nrows, tw.data(), s1, s2);
    return 0;
  });
}
template <typename T>
int plain_row_c2r(int M, cplx<T>* base, long long nrows, double scale, double* s1, double* s2) {
  return dispatch_row_c2r<T>(M, nrows, s1, s2, [&](auto) { PlainRowIO<T> io; io.base = base; io.scale = (T)scale; io.M_of = M; return io; });
}
template <typename T>
int xgather_row_c2r(int M, int nx, int ny, int tc, int rb, const cplx<T>* X, cplx<T>* W, double scale, double* s1, double* s2) {
  return dispatch_row_c2r<T>(M, (long long)nx * ny, s1, s2, [&](auto) { return xgather_row_io(X, W, scale, M, tc, rb, ny); });
}

// y pass in place on X (launch_col_xpose: whole columns), then the gathering z pass X -> W (+ moments)
template <typename T>
int xposed_yz(int nx, int ny, int nz, cplx<T>* X, cplx<T>* W, double* s1, double* s2) {
  constexpr int f64 = sizeof(T) == 8;
  const long long nzc = nz / 2;
  const int tc = col_tile_cols(f64, ny), rb = col_gen_row_block(f64, nx, g_rowblock);
  const ColGeom gy = xblock_y_geom(nx, ny, nzc, tc, rb);
  if (int rc = dispatch_col<T, +1>(ny, xpose_col_io<T>(X, gy, X, gy, (long long)nx * nzc, tc), (long long)nx * nzc)) return rc;
  return xgather_row_c2r<T>((int)nzc, nx, ny, tc, rb, X, W, 1.0 / ((double)nx * ny * nz), s1, s2);
}

template <class C>
void run_row_r2c(const PlainRowFwdIO<typename C::T>& io, long long nrows, const cplx<typename C::T>* tw) {
  using F = RowR2C<C, PlainRowFwdIO<typename C::T>>;
  using cx = cplx<typename C::T>;
  std::vector<cx> lds((size_t)C::LDS_BYTES / sizeof(cx));
  std::vector<typename F::Regs> regs(C::NT);
  const long long ntiles = (nrows + C::NRT - 1) / C::NRT;
  for (long long tile = 0; tile < ntiles; ++tile) {
    for (int t = 0; t < C::NT; ++t) F::prologue(t, tw, lds.data());
    const cx* ltw = F::lds_tw(lds.data());
    if (C::NPASS >= 2) for (int t = 0; t < C::NT; ++t) F::pass_first(t, tile, nrows, io, lds.data());
    if (C::NPASS == 3) {
      for (int t = 0; t < C::NT; ++t) F::pass_mid_read(t, ltw, lds.data(), regs[t]);
      for (int t = 0; t < C::NT; ++t) F::pass_mid_write(t, lds.data(), regs[t]);
    }
    // every thread reads all its LDS inputs before any thread stores (stores go to global memory only)
    for (int t = 0; t < C::NT; ++t) F::pass_last(t, tile, nrows, io, ltw, lds.data());
  }
}

template <typename T>
int dispatch_row_r2c(int M, cplx<T>* base, long long nrows) {
  auto tw = make_twiddles<T>(2 * M);
  PlainRowFwdIO<T> io; io.base = base; io.M_of = M;
  return for_row_size(M, -1, [&](auto m) { run_row_r2c<typename RowSel<T, decltype(m)::value>::type>(io, nrows, tw.data()); return 0; });
}

template <typename T>
int r2c_impl(int nx, int ny, int nz, const T* field, cplx<T>* K) {
  const long long nzc = nz / 2;
  std::vector<cplx<T>> W((size_t)nx * ny * nzc);
  memcpy(W.data(), field, W.size() * sizeof(cplx<T>));
  int rc = dispatch_row_r2c<T>((int)nzc, W.data(), (long long)nx * ny);
  if (rc) return rc;
  rc = plain_col_pass<T, -1>(ny, W.data(), y_geom(ny, nzc), (long long)nx * nzc);
  if (rc) return rc;
  rc = plain_col_pass<T, -1>(nx, W.data(), x_geom(ny, nzc), (long long)ny * nzc);
  if (rc) return rc;
  const int nzh = (int)nzc + 1;
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy) {
      const long long col = (long long)ix * ny + iy, mcol = (long long)((nx - ix) % nx) * ny + (ny - iy) % ny;
      for (int iz = 1; iz < nzc; ++iz) K[col * nzh + iz] = W[col * nzc + iz];
      const cplx<T> a = W[col * nzc], b = W[mcol * nzc];
      K[col * nzh] = mk<T>((T)0.5 * (a.x + b.x), (T)0.5 * (a.y - b.y));
      K[col * nzh + nzc] = mk<T>((T)0.5 * (a.y + b.y), (T)0.5 * (b.x - a.x));
    }
  return 0;
}

template <class C, int DIR>
void run_row_c2c(const ScaledRowIO<typename C::T>& io, long long nrows, const cplx<typename C::T>* tw) {
  using F = RowC2C<C, DIR, ScaledRowIO<typename C::T>>;
  using cx = cplx<typename C::T>;
  std::vector<cx> lds((size_t)C::LDS_BYTES / sizeof(cx) + 1);
  std::vector<typename F::Regs> regs(C::NT);
  const long long ntiles = (nrows + C::NRT - 1) / C::NRT;
  for (long long tile = 0; tile < ntiles; ++tile) {
    for (int t = 0; t < C::NT; ++t) F::prologue(t, tw, lds.data());
    const cx* ltw = F::lds_tw(lds.data());
    for (int t = 0; t < C::NT; ++t) F::pass_first(t, tile, nrows, io, lds.data());
    if (C::NPASS == 3) {
      for (int t = 0; t < C::NT; ++t) F::pass_mid_read(t, ltw, lds.data(), regs[t]);
      for (int t = 0; t < C::NT; ++t) F::pass_mid_write(t, lds.data(), regs[t]);
    }
    if (C::NPASS >= 2)
      for (int t = 0; t < C::NT; ++t) F::pass_last(t, tile, nrows, io, ltw, lds.data());
  }
}

template <typename T, int DIR>
int dispatch_row_c2c(int M, cplx<T>* base, long long nrows, double scale) {
  auto tw = make_twiddles<T>(M);
  ScaledRowIO<T> io; io.base = base; io.M_of = M; io.scale = (T)scale;
  return for_rowc_size(M, -1, [&](auto m) { run_row_c2c<typename RowSel<T, decltype(m)::value>::type, DIR>(io, nrows, tw.data()); return 0; });
}

// unpacked c2c in place on data[nx][ny][nz] (same pass order as rf_execute_c2c)
template <typename T, int DIR>
int c2c_impl(int nx, int ny, int nz, cplx<T>* W) {
  int rc = plain_col_pass<T, DIR>(nx, W, x_geom(ny, nz), (long long)ny * nz);
  if (rc) return rc;
  rc = plain_col_pass<T, DIR>(ny, W, y_geom(ny, nz), (long long)nx * nz);
  if (rc) return rc;
  return dispatch_row_c2c<T, DIR>(nz, W, (long long)nx * ny, DIR > 0 ? 1.0 / ((double)nx * ny * nz) : 1.0);
}

struct GenHost {
  SigmaTableHost tab;
  GenParams gp;
};

void fill_gen(GenHost& h, int nx, int ny, int nz, const double* kx2, const double* ky2, const double* kz2,
              const double* log10k, const double* sigma, int nt, int noise_mode, uint64_t seed, const double* noise) {
  build_sigma_table(log10k, sigma, nt, h.tab);
  GenParams& g = h.gp;
  g.nx = nx; g.ny = ny; g.nz = nz; g.kx2 = kx2; g.ky2 = ky2; g.kz2 = kz2;
  g.xt = h.tab.xt.data(); g.st = h.tab.st.data(); g.sl = h.tab.sl.data(); g.bin = h.tab.bin.data();
  g.nt = nt; g.nbins = (int)h.tab.bin.size(); g.x0 = h.tab.x0; g.inv_dx = h.tab.inv_dx;
  g.noise_mode = noise_mode; g.seed = seed; g.seed_dev = nullptr; g.noise = noise;
  g.zpitch = nz / 2 + 1; g.zoff = 0;
}
// the parameters of an x pass that reads an API-layout k array instead of generating
inline GenParams kspace_params(int nx, int ny, int nz) {
  GenParams gp;
  memset(&gp, 0, sizeof(gp));
  gp.nx = nx; gp.ny = ny; gp.nz = nz; gp.zpitch = nz / 2 + 1;
  return gp;
}

// the y and z passes behind an x pass that wrote `Wx` (W itself, or the blocked intermediate)
template <typename T>
int yz_passes(int nx, int ny, int nz, cplx<T>* Wx, cplx<T>* W, double* s1, double* s2) {
  const long long nzc = nz / 2;
  if (Wx != W) return xposed_yz<T>(nx, ny, nz, Wx, W, s1, s2);
  if (int rc = plain_col_pass<T, +1>(ny, W, y_geom(ny, nzc), (long long)nx * nzc)) return rc;
  return plain_row_c2r<T>((int)nzc, W, (long long)nx * ny, 1.0 / ((double)nx * ny * nz), s1, s2);
}

template <typename T>
int c2r_impl(int nx, int ny, int nz, const GenHost* gen, const cplx<T>* kspace, cplx<T>* W, double* s1, double* s2) {
  const long long nzc = nz / 2;
  // x pass (generation or API-layout k-space fused into the load), into W or the blocked intermediate
  const bool xp = xposed<T>(nx, ny, nzc);
  std::vector<cplx<T>> X(xp ? (size_t)nx * ny * nzc : 0);
  cplx<T>* Wx = xp ? X.data() : W;
  const GenColIO<T> gio = gen_col_io<T>(Wx, xp ? xposed_x_geom<T>(nx, ny, nzc) : x_geom(ny, nzc), gen ? gen->gp : kspace_params(nx, ny, nz), kspace, 0, (int)nzc);
  if (int rc = dispatch_col<T, +1, GenColIO<T>, GenSel>(nx, gio, (long long)ny * nzc)) return rc;
  return yz_passes<T>(nx, ny, nz, Wx, W, s1, s2);
}

// fix_fill_kernel (rf_kernels.h): the repaired kz = 0 slot of every mode (ix, iy) into the side buffer the FIX = 3 launch reads
template <class IOF, class CT>
void fill_fix_buffer(IOF iof, CT* buf) {
  const int nx = iof.gp.nx, ny = iof.gp.ny;
  std::vector<char> lds(IOF::LDS_EXTRA + 16);
  iof.bind_seed();
  iof.prologue(0, 1, lds.data());
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix) buf[(size_t)iy * nx + ix] = iof.fix_value((long long)iy * iof.nzl, ix, 0);
}

// One step of a fast generation pass as rf_col_gen_launch.h FastLaunch::step turns it into a launch: P = the variant's rf_select.h
// FastPassOf, the IO type by the step's io, the kernel by its kind; the tiles by fast_step_tile.
template <class P>
int run_fast_step(const FastIoArgs<typename P::T>& a, const FastStep& st, const cplx<typename P::T>* tw) {
  using C = typename P::C;
  auto one = [&](auto io) {
    if constexpr (P::HALVES) run_col2_pass<C, +1>(io, st, tw);
    else run_col_pass<C, +1>(io, st, tw);
    return 0;
  };
  switch (st.kind) {
    case FAST_FIX_FILL:
      if constexpr (P::side) { fill_fix_buffer(fast_col_io<typename P::IOF>(a), a.fixbuf); return 0; }
      return -2;
    case FAST_COLPAIR:
      if constexpr (P::pairs) {
        if (st.io == FAST_IO_LEAN) { run_colpair_pass<C, +1>(fast_col_io<typename P::IO0>(a), st, tw); return 0; }
        if (st.io == FAST_IO_FIRST) { run_colpair_pass<C, +1>(fast_col_io<typename P::IOC>(a), st, tw); return 0; }
      }
      return -2;
    default:
      return st.io == FAST_IO_LEAN ? one(fast_col_io<typename P::IO0>(a)) : st.io == FAST_IO_REPAIR ? one(fast_col_io<typename P::IO1>(a)) : one(fast_col_io<typename P::IOC>(a));
  }
}
// The variant and the launches of the native fast generation pass of a whole grid on one rank, as launch_col_fastgen chooses them:
// fastgen_variant, its FastListOf entry at length nx, fastgen_sequence.  f(Cfg<FastPassOf>{}, sequence); -2: the library refuses.
int g_pairs = 1;           // emu_set_pairs(0) clears FastPass::pairs: one tile per workgroup (ColFFT) where the library runs tile pairs
// What launch_col_fastgen (rf_k_col_gen.hip) is told besides the grid: pot 0 / 1 (a potential array is stored) / 2 (the pass transforms
// pscale delta(k) / k^2); src 0 native generator / 1 resident float64 deviates / 2 float32 pairs in the replay's runs (first: the
// exclusive scan of the per-segment counts, nseg + 1 entries; cap: slots per segment); the rows [x0, x1) that are kept (replicated
// generation: x0 > 0 or x1 < nx) and the kz planes [kz0, kz0 + nzl) of a kz-slab rank.  The defaults are one rank's whole grid.
struct FastCall {
  int pot = 0;
  double pscale = 1.0;
  int src = 0;
  const double* noise64 = nullptr;
  const cplx<float>* noise32 = nullptr;
  const unsigned long long* first = nullptr;
  int nseg = 0;
  unsigned long long cap = 0;
  int x0 = 0, x1 = 1 << 30, kz0 = 0, nzl = -1;       // nzl < 0: all nz / 2 planes
  bool loads = false;                                // the pass's loads alone (fast_loads), no transform
  bool slab(int nx) const { return x0 > 0 || x1 < nx; }
  FastVariant variant(int f64, int nx) const { return fastgen_variant(f64, nx, pot == 2, src == 1, src == 2, pot == 1, slab(nx)); }
};
// The cells one variant's pass LOADS -- what its IO generates for row r of column C, the kz = 0 slot replaced by the owning lane's
// repair as ColFFT::pass_first replaces it (FIX = 1) -- with no transform behind them: out [N][ncols], row = mode index ix
template <class P>
int fast_loads(const FastIoArgs<typename P::T>& a, long long ncols, cplx<typename P::T>* out) {
  using C = typename P::C;
  using IO = typename P::IO1;
  using V = V16<typename P::T>;
  constexpr int L = C::N / C::R1;
  IO io = fast_col_io<IO>(a);
  std::vector<char> lds(IO::LDS_EXTRA + 16);
  io.bind_seed();
  io.prologue(0, 1, lds.data());
  for (int phase = 0; phase < (P::HALVES ? 2 : 1); ++phase) {
    if constexpr (P::HALVES) io.set_phase(phase);
    for (long long C0 = 0; C0 < ncols; C0 += V::CPL)
      for (int r = 0; r < C::N; ++r) {
        const int rb = r % L, ro = r - rb;
        V v = io.load(C0, 0, rb, ro);
        if (io.needs_fix(C0)) v.c[0] = io.fix_value(C0, rb, ro);
        const long long ix = P::HALVES ? 2 * r + phase : r;
        for (int k = 0; k < V::CPL; ++k) out[ix * ncols + C0 + k] = v.c[k];
      }
  }
  return 0;
}
template <typename T, class F>
int with_fast_pass(int nx, const ColGeom& g, long long ncols, int nzl, const FastCall& c, F&& f) {
  const FastVariant v = c.variant(sizeof(T) == 8, nx);
  return with_fast_variant(FastListOf<T>{}, v, -2, [&](auto e) {
    return FastGen<T>::template at<decltype(e)>(nx, -2, [&](auto k) {
      using P = typename decltype(k)::type;
      if (!P::accepts(g, ncols, nzl, c.x0, c.x1)) return -2;
      FastPass pass = P::pass;
      if (!g_pairs) pass.pairs = false;
      const FastSequence q = fastgen_sequence(pass, nzl, ncols, c.kz0, P::full_rows(c.x0, c.x1), g, true);
      return q.valid ? f(k, q) : -2;
    });
  });
}

// The x pass of one call -- one rank's rows [x0, x1) and planes [kz0, kz0 + nzl) -- into the whole grid's intermediate
// W [nx][ny][nz / 2] (Wx: the blocked intermediate instead, whole-grid calls only), and its potential array P [nx][ny][ppitch] (pot = 1).
template <typename T>
int fast_x_pass(int nx, int ny, int nz, const GenHost& h, uint64_t seed, double xlo, double xhi, double dkx, const FastCall& c,
                cplx<T>* W, cplx<T>* Wx, cplx<T>* P) {
  constexpr int f64 = sizeof(T) == 8;
  const long long nzc = nz / 2;
  const int nzl = c.nzl < 0 ? (int)nzc : c.nzl;
  const long long ncols = (long long)ny * nzl;
  const bool whole_z = c.kz0 == 0 && nzl == nzc;
  if (nzl <= 0 || c.kz0 < 0 || c.kz0 + nzl > nzc || (c.src != 0 && !whole_z) || (Wx != W && (!whole_z || c.slab(nx)))) return -2;
  if (c.loads && (Wx != W || c.slab(nx))) return -2;
  if ((c.pot == 1) != (P != nullptr) || (c.src == 1 && !c.noise64) || (c.src == 2 && !(c.noise32 && c.first && c.nseg > 0))) return -2;
  std::vector<FastRec> rec;
  FastGenParams f;
  memset(&f, 0, sizeof(f));
  double x0, dx;
  if (!build_fast_records(h.tab, xlo, xhi, rec, x0, dx)) return -3;
  if ((int)rec.size() > FAST_LDS_BINS) return -3;          // as build_fast (rf_capi.hip): such a plan runs the exact kernel
  f.nx = nx; f.ny = ny; f.nz = nz; f.dkx = (float)dkx; f.dky = (float)std::sqrt(h.gp.ky2[1]); f.dkz = (float)std::sqrt(h.gp.kz2[1]);
  f.rec = rec.data(); f.nbins = (int)rec.size();
  f.u_scale = (float)(0.5 * std::log10(2.0) / dx); f.u_off = (float)(-x0 / dx);
  // the side arrays of a rank: its own planes, then the Nyquist plane (make_fast and rf_plan_create, rf_capi.hip)
  f.seed = seed; f.zpitch = nzl + 1; f.zoff = c.kz0; f.ppitch = f64 ? nzl + 1 : nzl + (nzl >= 256 ? 64 : 2);
  f.pscale = c.pscale; f.emit_potential = c.pot == 2 ? 1 : 0;
  std::vector<RowLoc> rowtab;
  if (c.src == 1) f.noise = c.noise64;
  if (c.src == 2) {                                        // mt_rowtab_kernel: entry iy nx + ix
    int bad = 0;
    rowtab.resize((size_t)nx * ny);
    for (int ix = 0; ix < nx; ++ix)
      for (int iy = 0; iy < ny; ++iy)
        rowtab[(size_t)iy * nx + ix] = make_rowloc(c.first, c.nseg, ((unsigned long long)ix * ny + iy) * (unsigned)(nzc + 1), (unsigned)(nzc + 1), &bad);
    if (bad) return -4;
    f.noise32 = c.noise32; f.rowtab = rowtab.data(); f.seg_cap = c.cap;
  }
  // a kz slab is generated into an array of its own planes, as on its rank, and copied into the whole grid's
  std::vector<cplx<T>> own(whole_z ? 0 : (size_t)nx * ny * nzl), fixbuf((size_t)nx * ny);
  const ColGeom g = Wx != W ? xposed_x_geom<T>(nx, ny, nzc) : x_geom(ny, nzl);
  cplx<T>* dst = Wx != W ? Wx : whole_z ? W : own.data();
  if (c.x0 > 0) dst += (long long)c.x0 * g.row_stride;     // (fast_col_io moves the base back by x0 rows: row x0 lands on row x0 of W)
  const FastIoArgs<T> a{f, dst, g, c.kz0, nzl, c.x0, c.x1, P, fixbuf.data()};
  g_fast_steps.clear();
  auto tw = make_twiddles<T>(nx);
  g_count_visits = true;
  const int rc = with_fast_pass<T>(nx, a.g, ncols, nzl, c, [&](auto k, const FastSequence& q) {
    g_fast_visits.assign((size_t)(ncols / decltype(k)::type::C::TC), 0);
    if (c.loads) return fast_loads<typename decltype(k)::type>(a, ncols, dst);
    for (int i = 0; i < q.n; ++i) {
      g_fast_steps.push_back(q.step[i]);
      if (int e = run_fast_step<typename decltype(k)::type>(a, q.step[i], tw.data())) return e;
    }
    return 0;
  });
  g_count_visits = false;
  if (rc) return rc;
  if (!whole_z)
    for (long long col = 0; col < (long long)nx * ny; ++col)
      std::copy(own.begin() + col * nzl, own.begin() + (col + 1) * nzl, W + col * nzc + c.kz0);
  return 0;
}

// finish: the y and z passes behind the x pass (the last of the calls that fill W between them)
template <typename T>
int realise_fast_impl(int nx, int ny, int nz, const GenHost& h, uint64_t seed, double xlo, double xhi, double dkx, const FastCall& c,
                      bool finish, cplx<T>* W, cplx<T>* P, double* s1, double* s2) {
  const long long nzc = nz / 2;
  const bool whole = c.kz0 == 0 && (c.nzl < 0 || c.nzl == nzc) && !c.slab(nx);
  const bool xp = whole && finish && !c.loads && xposed<T>(nx, ny, nzc);
  std::vector<cplx<T>> X(xp ? (size_t)nx * ny * nzc : 0);
  cplx<T>* Wx = xp ? X.data() : W;
  if (int rc = fast_x_pass<T>(nx, ny, nz, h, seed, xlo, xhi, dkx, c, W, Wx, P)) return rc;
  return finish && !c.loads ? yz_passes<T>(nx, ny, nz, Wx, W, s1, s2) : 0;
}


// ---- non-power-of-two path (rf_generic.h): the same block functions the kernels run ----
// One "thread" per block by default (tid, nth) = (0, 1) with a no-op barrier; with emu_set_generic_threads(nth > 1) every block is run by
// nth host threads that share the block's LDS image and meet at a real barrier wherever the kernels call __syncthreads() -- the
// kernels' own thread walk (GenericWalk::fixed when nth % tile == 0), four loads in flight, per-thread stores and barrier placement.
struct NoSync { void operator()() const {} };
struct BarrierSync {
  pthread_barrier_t* bar;
  void operator()() const { pthread_barrier_wait(bar); }
};

// The library's sequences (rf_generic.h generic_*_seq) with every launch replaced by a loop over its blocks.
// g_generic_cap: the longest line kept "in LDS" -- the library's cap is 8192 / 4096; tests lower it so that small grids take the
// four-step form of the long axes.
int g_generic_cap = 0;                  // 0: generic_max_axis(dtype)
int g_generic_tile = 3;                 // lines per block of the strided passes: 3 = deliberately not dividing the line counts (the walk by
                                        // index); 1 = the kernels' walk, a thread staying on one line (GenericWalk::fixed)
int g_generic_threads = 1;              // host threads per block (1: the single-thread emulation)
int g_generic_prefer_split = 1;         // 1: a strided line that fits but prefers the four-step form runs it, as in the library (rf_generic.h
                                        // generic_axis_form); 0: every line that fits the cap is one line
// a strided pass stages its stage and position tables behind the line image(s) unless even ONE line leaves no room for them
// (rf_k_generic.hip strided_shape's last resort: the longest lines that are not smooth)
inline int generic_tables_fit(const GenericAxis& ax, int elem_bytes) {
  return (size_t)generic_bufs(ax) * ax.n * elem_bytes + generic_extra_bytes(ax, elem_bytes) <= (size_t)GENERIC_LDS_MAX ? 1 : 0;
}

// body(tid, sync) on g_generic_threads host threads (thread 0 is the caller); body loops over the blocks of one launch itself and
// calls sync() after each block, which stands for the workgroup boundary: the LDS image is reused by the next block
template <class Body> void run_generic_threads(Body body) {
  const int nth = g_generic_threads;
  if (nth <= 1) { body(0, NoSync()); return; }
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, nullptr, (unsigned)nth);
  std::vector<std::thread> pool;
  for (int t = 1; t < nth; ++t) pool.emplace_back([&body, &bar, t] { body(t, BarrierSync{&bar}); });
  body(0, BarrierSync{&bar});
  for (auto& th : pool) th.join();
  pthread_barrier_destroy(&bar);
}

template <typename T> struct EmuGenericOps {
  const cplx<T>*rx, *ry, *rz;
  int nx, ny, nz, M;                    // M = row length of the contiguous complex transform's root table / 2 (packed) -- see callers
  long long rows;
  // the block's LDS: exactly the bytes the launchers ask for with the stage and position tables switched on (rf_k_generic.hip
  // strided_shape / row_shape), on the heap -- an index past them is a heap overrun for AddressSanitizer
  std::unique_ptr<unsigned char[]> lds_raw;
  double s1 = 0, s2 = 0;
  const cplx<T>* root(int which) const { return which == 0 ? rx : (which == 1 ? ry : rz); }
  cplx<T>* lds_image(const GenericAxis& ax, int pitch) {
    const size_t bytes = (size_t)generic_bufs(ax) * ax.n * pitch * sizeof(cplx<T>) + generic_extra_bytes(ax, (int)sizeof(cplx<T>));
    lds_raw.reset(new unsigned char[bytes]);
    return reinterpret_cast<cplx<T>*>(lds_raw.get());
  }
  int nthreads() const { return g_generic_threads > 1 ? g_generic_threads : 1; }
  // rows per block of the contiguous passes: 2 for the single thread; the kernels' 8 / 4 (rows_per_block) with threads
  int row_tile() const { return g_generic_threads > 1 ? (g_generic_tile < 8 ? g_generic_tile : 8) : 2; }
  // one strided pass whose elements come from `from` (rf_generic.h generic_axis_block_from), block after block
  template <class Source>
  int axis_source(Source from, void* dst, const GenericAxis& ax, long long stride, long long inner, long long outer, long long nlines, int which, int sign, double scale) {
    const int TC = g_generic_tile, nth = nthreads(), tw = generic_tables_fit(ax, (int)sizeof(cplx<T>));
    cplx<T>* lds = lds_image(ax, TC);
    run_generic_threads([&](int tid, auto sync) {
      for (long long b = 0; b * TC < nlines; ++b) {
        generic_axis_block_from<T>(from, (cplx<T>*)dst, ax, stride, inner, outer, nlines, TC, root(which), sign, (T)scale, lds, b, tid, nth, sync, tw);
        sync();
      }
    });
    return 0;
  }
  int axis(const void* src, void* dst, const GenericAxis& ax, long long stride, long long inner, long long outer, long long nlines, int which, int sign, double scale) {
    return axis_source(GenericMemSource<T>((const cplx<T>*)src, stride, inner, outer), dst, ax, stride, inner, outer, nlines, which, sign, scale);
  }
  // generic_c2r_from_seq: the Source and the cell of a descriptor -- the generator, or a component of the gradient / Hessian of S
  static GenericGenSource<T> source(const GenParams& gp, const void*) { return GenericGenSource<T>(gp, gp.seed); }
  template <class P> static GenericDerivSource<T, P> source(const P& dp, const void* S) { return GenericDerivSource<T, P>(dp, (const cplx<T>*)S); }
  static cplx<T> cell(const GenParams& gp, const void*, long long, int ix, int iy, int iz) { return gen_cell<T>(gp, gp.seed, ix, iy, iz); }
  template <class P> static cplx<T> cell(const P& dp, const void* S, long long row, int ix, int iy, int iz) {
    return deriv_cell<T>(dp, ((const cplx<T>*)S)[row * dp.pitch + iz], ix, iy, iz);
  }
  template <class From>
  int axis_from(const From& from, const void* S, void* dst, const GenericAxis& ax, long long stride, long long inner, long long outer, long long nlines, int which, int sign, double scale) {
    return axis_source(source(from, S), dst, ax, stride, inner, outer, nlines, which, sign, scale);
  }
  // ... and the cells alone, API layout (the loop of gen_kspace_kernel / the elementwise derivative kernel; S == K is allowed)
  template <class From>
  int materialise(const From& from, const void* S, void* K) {
    const int nzh = from.nz / 2 + 1;
    for (int ix = 0; ix < from.nx; ++ix)
      for (int iy = 0; iy < from.ny; ++iy) {
        const long long row = (long long)ix * from.ny + iy;
        for (int iz = 0; iz < nzh; ++iz) ((cplx<T>*)K)[row * nzh + iz] = cell(from, S, row, ix, iy, iz);
      }
    return 0;
  }
  int lines(const void* src, void* dst, const GenericLines& L, int which) {
    const int TC = g_generic_tile, nth = nthreads(), tw = generic_tables_fit(L.ax, (int)sizeof(cplx<T>));
    cplx<T>* lds = lds_image(L.ax, TC);
    run_generic_threads([&](int tid, auto sync) {
      for (long long b = 0; b * TC < L.nlines(); ++b) {
        generic_lines_block<T>((const cplx<T>*)src, (cplx<T>*)dst, L, TC, root(which), lds, b, tid, nth, sync, tw);
        sync();
      }
    });
    return 0;
  }
  GenericAxis az;
  int row_c2r(const void* G, void* W, double scale) {
    const int TR = row_tile(), nth = nthreads();
    cplx<T>* lds = lds_image(az, generic_row_pitch(TR));
    std::vector<double> p1(nth, 0.0), p2(nth, 0.0);          // every thread's share of (sum, sum of squares)
    run_generic_threads([&](int tid, auto sync) {
      double a1 = 0, a2 = 0;
      for (long long b = 0; b * TR < rows; ++b) {
        generic_row_c2r_block<T>((const cplx<T>*)G, (T*)W, az, rows, TR, rz, (T)scale, lds, b, tid, nth, sync, a1, a2, 1);
        sync();
      }
      p1[tid] = a1; p2[tid] = a2;
    });
    for (int t = 0; t < nth; ++t) { s1 += p1[t]; s2 += p2[t]; }      // in thread order: deterministic
    return 0;
  }
  int row_r2c(const void* W, void* G) {
    const int TR = row_tile(), nth = nthreads();
    cplx<T>* lds = lds_image(az, generic_row_pitch(TR));
    run_generic_threads([&](int tid, auto sync) {
      for (long long b = 0; b * TR < rows; ++b) {
        generic_row_r2c_block<T>((const T*)W, (cplx<T>*)G, az, rows, TR, rz, lds, b, tid, nth, sync, 1);
        sync();
      }
    });
    return 0;
  }
  int untangle(const void* G, void* Z) { for (long long i = 0; i < rows * M; ++i) generic_untangle_at<T>((const cplx<T>*)G, (cplx<T>*)Z, M, rz, i); return 0; }
  int tangle(const void* Z, void* G) { for (long long i = 0; i < rows * (M + 1); ++i) generic_tangle_at<T>((const cplx<T>*)Z, (cplx<T>*)G, M, rz, i); return 0; }
  int moments(const void* W) {
    const T* w = (const T*)W;
    for (long long i = 0; i < rows * 2 * M; ++i) { s1 += (double)w[i]; s2 += (double)w[i] * (double)w[i]; }
    return 0;
  }
  int copy(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
};
// the form of every axis by the library's rule (rf_generic.h generic_axis_form: x and y are strided, the contiguous axis is not), with the
// emulator's cap and switch
template <typename T> bool emu_dims(int nx, int ny, int nz, bool packed, GenericDims& d) {
  const int cap = g_generic_cap > 0 ? g_generic_cap : generic_max_axis(sizeof(T) == 8);
  const bool prefer = g_generic_prefer_split != 0;
  d.nx = nx; d.ny = ny; d.nz = nz; d.csize = sizeof(cplx<T>);
  if (packed && (nz & 1)) return false;
  return generic_axis_form(nx, cap, (int)d.csize, true, d.ax, d.lx, prefer) && generic_axis_form(ny, cap, (int)d.csize, true, d.ay, d.ly, prefer) &&
         generic_axis_form(packed ? nz / 2 : nz, cap, (int)d.csize, false, d.az, d.lz, prefer);
}
// the form of one axis as 32 ints: n1, n2 (0, 0: one line) and, per line (the whole line, or the sub-lines n1 then n2; the second block
// zero for one line), nf, smooth, whether the stage tables fit behind one line's image(s), and the 12 radices
inline void emu_form_line(const GenericAxis& ax, int elem_bytes, int* out15) {
  out15[0] = ax.nf; out15[1] = ax.smooth; out15[2] = generic_tables_fit(ax, elem_bytes);
  for (int s = 0; s < GENERIC_MAX_FACTORS; ++s) out15[3 + s] = s < ax.nf ? ax.f[s] : 0;
}
inline void emu_form_out(const GenericAxis& ax, const GenericLong& lg, int elem_bytes, int* out32) {
  std::fill(out32, out32 + 32, 0);
  if (lg.split()) { out32[0] = lg.n1; out32[1] = lg.n2; emu_form_line(lg.a1, elem_bytes, out32 + 2); emu_form_line(lg.a2, elem_bytes, out32 + 17); }
  else emu_form_line(ax, elem_bytes, out32 + 2);
}

template <typename T>
int generic_c2r_impl(int nx, int ny, int nz, const cplx<T>* K, T* W, double* s1, double* s2) {
  GenericDims d;
  if (!emu_dims<T>(nx, ny, nz, true, d)) return -1;
  const long long nzh = nz / 2 + 1;
  auto rx = make_twiddles<T>(nx), ry = make_twiddles<T>(ny), rz = make_twiddles<T>(nz);
  std::vector<cplx<T>> G((size_t)nx * ny * nzh), G2((size_t)nx * ny * nzh);
  EmuGenericOps<T> ops{rx.data(), ry.data(), rz.data(), nx, ny, nz, nz / 2, (long long)nx * ny, nullptr};
  ops.az = d.az;
  const int rc = generic_c2r_seq(ops, d, K, G.data(), G2.data(), W, 1.0 / ((double)nx * ny * nz));
  if (s1) *s1 = ops.s1;
  if (s2) *s2 = ops.s2;
  return rc;
}

// generic_c2r_impl with the first pass taking its cells from a descriptor (rf_generic.h generic_c2r_from_seq; an x axis beyond the cap:
// its unfused fallback): a realisation with the generation inside the x pass (GenParams), or one component of the gradient / Hessian of
// the potential S as a field with the factor applied there (GradParams / HessParams)
template <typename T, class From>
int generic_c2r_from_impl(int nx, int ny, int nz, const From& from, const void* S, T* W, double* s1, double* s2) {
  GenericDims d;
  if (!emu_dims<T>(nx, ny, nz, true, d)) return -1;
  const long long nzh = nz / 2 + 1;
  auto rx = make_twiddles<T>(nx), ry = make_twiddles<T>(ny), rz = make_twiddles<T>(nz);
  std::vector<cplx<T>> G((size_t)nx * ny * nzh), G2((size_t)nx * ny * nzh);
  EmuGenericOps<T> ops{rx.data(), ry.data(), rz.data(), nx, ny, nz, nz / 2, (long long)nx * ny, nullptr};
  ops.az = d.az;
  const int rc = generic_c2r_from_seq(ops, d, from, S, G.data(), G2.data(), W, 1.0 / ((double)nx * ny * nz));
  if (s1) *s1 = ops.s1;
  if (s2) *s2 = ops.s2;
  return rc;
}
// the parameters of a component as the emulator's exports take them; false: refused (bad shape, axes, pitch, or divide without tables)
template <class P>
bool emu_deriv_params(int nx, int ny, int nz, int divide, const double* kx2, const double* ky2, const double* kz2, long long spitch, P& g) {
  g.nx = nx; g.ny = ny; g.nz = nz; g.divide = divide != 0;
  g.kx2 = kx2; g.ky2 = ky2; g.kz2 = kz2; g.pitch = spitch;
  return nx >= 1 && ny >= 1 && nz >= 2 && !(nz & 1) && deriv_valid(g) && !(divide && !(kx2 && ky2 && kz2));
}
inline bool emu_grad_params(int nx, int ny, int nz, int axis, double scale, double dk, int divide, const double* kx2, const double* ky2, const double* kz2,
                            long long spitch, GradParams& g) {
  memset(&g, 0, sizeof(g));
  g.axis = axis; g.sdk = scale * dk;
  return emu_deriv_params(nx, ny, nz, divide, kx2, ky2, kz2, spitch, g);
}
inline bool emu_hess_params(int nx, int ny, int nz, int a, int b, double scale, double dk_a, double dk_b, int divide, const double* kx2, const double* ky2,
                            const double* kz2, long long spitch, HessParams& g) {
  memset(&g, 0, sizeof(g));
  g.a = a; g.b = b; g.sdk2 = -scale * dk_a * dk_b;
  return emu_deriv_params(nx, ny, nz, divide, kx2, ky2, kz2, spitch, g);
}
// K = the component alone, W = its field: the bodies of the four exports below
template <class P> int emu_deriv_k(int f64, const P& g, const void* S, void* K) {
  if (f64) { EmuGenericOps<double> ops{}; return ops.materialise(g, S, K); }
  EmuGenericOps<float> ops{};
  return ops.materialise(g, S, K);
}
template <class P> int emu_deriv_c2r(int f64, const P& g, const void* S, void* W, double* s1, double* s2) {
  return f64 ? generic_c2r_from_impl<double>(g.nx, g.ny, g.nz, g, S, (double*)W, s1, s2) : generic_c2r_from_impl<float>(g.nx, g.ny, g.nz, g, S, (float*)W, s1, s2);
}
template <typename T>
int lpt2_accumulate_impl(int step, T* H, T* Tacc, T* Sacc, long long n) {
  for (long long i = 0; i < n; ++i) {
    switch (step) {
      case LPT2_FIRST: lpt2_step<T, LPT2_FIRST>(H[i], Tacc[i], Sacc[i]); break;
      case LPT2_DIAG2: lpt2_step<T, LPT2_DIAG2>(H[i], Tacc[i], Sacc[i]); break;
      case LPT2_DIAG3: lpt2_step<T, LPT2_DIAG3>(H[i], Tacc[i], Sacc[i]); break;
      case LPT2_OFF: lpt2_step<T, LPT2_OFF>(H[i], Tacc[i], Sacc[i]); break;
      case LPT2_LAST: lpt2_step<T, LPT2_LAST>(H[i], Tacc[i], Sacc[i]); break;
      default: return -1;
    }
  }
  return 0;
}

// ---- particles (rf_core.h cic_*): the cloud-in-cell paint as rf_k_particles.hip runs it, on nth real host threads that add with
// __atomic operations to the shared accumulator grid and -- in the tiled form -- to the brick's shared tile image
template <class Body> void run_threads(int nth, Body body) {
  if (nth <= 1) { body(0, NoSync()); return; }
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, nullptr, (unsigned)nth);
  std::vector<std::thread> pool;
  for (int t = 1; t < nth; ++t) pool.emplace_back([&body, &bar, t] { body(t, BarrierSync{&bar}); });
  body(0, BarrierSync{&bar});
  for (auto& th : pool) th.join();
  pthread_barrier_destroy(&bar);
}
inline void atomic_add_u64(unsigned long long* p, uint64_t w) { __atomic_fetch_add(p, (unsigned long long)w, __ATOMIC_RELAXED); }

// The assignment scheme of an operation: the per-axis type, how a particle is located, and the rf_core.h functions that visit its cells
// -- cloud in cell (cic_*, eight cells) or the triangular-shaped cloud (tsc_*, 27), the functions rf_k_particles.hip's policies call.
struct EmuCic {
  typedef CicAxis Axis;
  template <typename T> static bool locate(T sx, T sy, T sz, const CicGrid& g, int ix, int iy, int iz, Axis& x, Axis& y, Axis& z) {
    return cic_particle<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
  }
  template <class... A> static void scatter_global(A&&... a) { cic_scatter_global(std::forward<A>(a)...); }
  template <class... A> static void scatter_tiled(A&&... a) { cic_scatter_tiled(std::forward<A>(a)...); }
  template <class... A> static double gather_global(A&&... a) { return cic_gather_global(std::forward<A>(a)...); }
  template <class... A> static double gather_tiled(A&&... a) { return cic_gather_tiled(std::forward<A>(a)...); }
};
struct EmuTsc {
  typedef TscAxis Axis;
  template <typename T> static bool locate(T sx, T sy, T sz, const CicGrid& g, int ix, int iy, int iz, Axis& x, Axis& y, Axis& z) {
    return tsc_particle<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
  }
  template <class... A> static void scatter_global(A&&... a) { tsc_scatter_global(std::forward<A>(a)...); }
  template <class... A> static void scatter_tiled(A&&... a) { tsc_scatter_tiled(std::forward<A>(a)...); }
  template <class... A> static double gather_global(A&&... a) { return tsc_gather_global(std::forward<A>(a)...); }
  template <class... A> static double gather_tiled(A&&... a) { return tsc_gather_tiled(std::forward<A>(a)...); }
};
// the same two schemes with the half-cell shift of an interlaced paint's second grid (rf_core.h cic_axis_half; the HALF instantiations of
// rf_k_particles.hip's paint operations): only how a particle is located differs
struct EmuCicHalf : EmuCic {
  template <typename T> static bool locate(T sx, T sy, T sz, const CicGrid& g, int ix, int iy, int iz, Axis& x, Axis& y, Axis& z) {
    return cic_particle_half<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
  }
};
struct EmuTscHalf : EmuTsc {
  template <typename T> static bool locate(T sx, T sy, T sz, const CicGrid& g, int ix, int iy, int iz, Axis& x, Axis& y, Axis& z) {
    return tsc_particle_half<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
  }
};

// The two walks of rf_k_particles.hip over an operation Op -- what it does before a brick's particles (prologue), with one particle's
// eight cells, with a dropped particle and after the brick (epilogue), over a tile of Op::Cell.  cic_global_kernel: one "lane" per particle.
template <typename T, class Op>
void cic_walk_global(const CicGrid& g, const T* sx, const T* sy, const T* sz, int nth, Op& op, unsigned long long* dropped) {
  const long long n = (long long)g.nx * g.ny * g.nz;
  *dropped = 0;
  run_threads(nth, [&](int tid, auto sync) {
    unsigned long long nd = 0;
    for (long long i = tid; i < n; i += nth) {
      int ix, iy, iz;
      cic_lattice(i, g.ny, g.nz, ix, iy, iz);
      typename Op::Scheme::Axis x, y, z;
      if (!Op::Scheme::template locate<T>(sx[i], sy[i], sz[i], g, ix, iy, iz, x, y, z)) { ++nd; op.dropped(i); continue; }
      op.particle(i, x, y, z, g);
    }
    if (nd) atomic_add_u64(dropped, nd);
  });
}
// cic_tiled_kernel: bricks one after the other, the threads of a brick share its tile image and meet at the kernel's barriers (and
// once more before the next brick takes the tile)
template <typename T, class Op>
void cic_walk_bricks(const CicGrid& g, const T* sx, const T* sy, const T* sz, int bx, int by, int bz, int halo, int nth, Op& op, unsigned long long* dropped) {
  std::vector<typename Op::Cell> image((size_t)cic_brick_tile(0, 1, 1, bx, by, bz, halo).cells());
  typename Op::Cell* tile = image.data();
  const int nbx = (g.nx + bx - 1) / bx, nby = (g.ny + by - 1) / by, nbz = (g.nz + bz - 1) / bz;
  *dropped = 0;
  run_threads(nth, [&](int tid, auto sync) {
    unsigned long long nd = 0;
    for (int b = 0; b < nbx * nby * nbz; ++b) {
      const CicTile t = cic_brick_tile((unsigned)b, nby, nbz, bx, by, bz, halo);
      op.prologue(tile, t, g, tid, nth);
      sync();
      for (int row = tid; row < bx * by; row += nth) {
        const int lx = row / by, ly = row - lx * by, ix = t.x0 + lx, iy = t.y0 + ly;
        for (int lz = 0; lz < bz; ++lz) {
          const int iz = t.z0 + lz;
          if (ix >= g.nx || iy >= g.ny || iz >= g.nz) continue;
          const long long i = ((long long)ix * g.ny + iy) * g.nz + iz;
          typename Op::Scheme::Axis x, y, z;
          if (!Op::Scheme::template locate<T>(sx[i], sy[i], sz[i], g, ix, iy, iz, x, y, z)) { ++nd; op.dropped(i); continue; }
          op.particle(i, x, y, z, lx, ly, lz, tile, t, g);
        }
      }
      sync();
      op.epilogue(tile, t, g, tid, nth);
      sync();
    }
    if (nd) atomic_add_u64(dropped, nd);
  });
}

// PaintOp: the threads add with __atomic operations to the shared accumulator grid and to the brick's shared tile image
template <class S>
struct EmuPaintOp {
  typedef unsigned long long Cell;
  typedef S Scheme;
  typedef typename S::Axis Axis;
  unsigned long long* A;
  void prologue(Cell* tile, const CicTile& t, const CicGrid&, int tid, int nth) const {
    for (int s = tid; s < t.cells(); s += nth) tile[s] = 0ull;
  }
  void particle(long long, const Axis& x, const Axis& y, const Axis& z, const CicGrid& g) const {
    S::scatter_global(x, y, z, g.ny, g.nz, [&](long long cell, uint64_t w) { atomic_add_u64(A + cell, w); });
  }
  void particle(long long, const Axis& x, const Axis& y, const Axis& z, int lx, int ly, int lz, Cell* tile, const CicTile& t, const CicGrid& g) const {
    S::scatter_tiled(x, y, z, lx, ly, lz, t, g.ny, g.nz, [&](int slot, uint64_t w) { atomic_add_u64(&tile[slot], w); },
                     [&](long long cell, uint64_t w) { atomic_add_u64(A + cell, w); });
  }
  void dropped(long long) const {}
  void epilogue(Cell* tile, const CicTile& t, const CicGrid& g, int tid, int nth) const {
    for (int s = tid; s < t.cells(); s += nth)
      if (tile[s]) atomic_add_u64(A + cic_tile_cell(t, s, g.nx, g.ny, g.nz), tile[s]);
  }
};
// GatherOp: every particle writes its own element of G, so the threads share nothing but the tile image (filled before a barrier,
// read-only after it) and the drop counter
template <typename T, class S>
struct EmuGatherOp {
  typedef T Cell;
  typedef S Scheme;
  typedef typename S::Axis Axis;
  const T* W;
  T* G;
  double coeff;
  int first;
  void prologue(Cell* tile, const CicTile& t, const CicGrid& g, int tid, int nth) const {
    for (int s = tid; s < t.cells(); s += nth) tile[s] = W[cic_tile_cell(t, s, g.nx, g.ny, g.nz)];
  }
  void out(long long i, double v) const { G[i] = cic_gather_out<T>(first != 0, coeff, v, first ? (T)0 : G[i]); }
  void particle(long long i, const Axis& x, const Axis& y, const Axis& z, const CicGrid& g) const {
    out(i, S::gather_global(x, y, z, g.ny, g.nz, [&](long long cell) { return (double)W[cell]; }));
  }
  void particle(long long i, const Axis& x, const Axis& y, const Axis& z, int lx, int ly, int lz, const Cell* tile, const CicTile& t,
                const CicGrid& g) const {
    out(i, S::gather_tiled(x, y, z, lx, ly, lz, t, g.ny, g.nz, [&](int slot) { return (double)tile[slot]; }, [&](long long cell) { return (double)W[cell]; }));
  }
  void dropped(long long i) const { if (first) G[i] = (T)0; }
  void epilogue(Cell*, const CicTile&, const CicGrid&, int, int) const {}
};
// what the tiled paint does with these particles, counted with the kernel's own rule (cic_scatter_tiled) by one thread: particles that
// leave their brick's tile, their adds straight into A, and the non-zero tile cells the bricks flush
template <class S>
struct EmuTileStatsOp {
  typedef unsigned long long Cell;
  typedef S Scheme;
  typedef typename S::Axis Axis;
  unsigned long long fallback = 0, fallback_adds = 0, flushed = 0;
  void prologue(Cell* tile, const CicTile& t, const CicGrid&, int, int) { std::fill(tile, tile + t.cells(), 0ull); }
  void particle(long long, const Axis& x, const Axis& y, const Axis& z, int lx, int ly, int lz, Cell* tile, const CicTile& t, const CicGrid& g) {
    const unsigned long long before = fallback_adds;
    S::scatter_tiled(x, y, z, lx, ly, lz, t, g.ny, g.nz, [&](int slot, uint64_t w) { tile[slot] += w; }, [&](long long, uint64_t) { ++fallback_adds; });
    if (fallback_adds != before) ++fallback;
  }
  void dropped(long long) {}
  void epilogue(Cell* tile, const CicTile& t, const CicGrid&, int, int) { flushed += t.cells() - std::count(tile, tile + t.cells(), 0ull); }
};

template <typename T, class Op>
int particles_walk(int nx, int ny, int nz, const T* sx, const T* sy, const T* sz, const double* inv_h, int form, int bx, int by, int bz, int halo, int nth,
                   Op op, unsigned long long* dropped) {
  const CicGrid g = {nx, ny, nz, {inv_h[0], inv_h[1], inv_h[2]}};
  if (form == 1) cic_walk_global(g, sx, sy, sz, nth, op, dropped);
  else cic_walk_bricks(g, sx, sy, sz, bx, by, bz, halo, nth, op, dropped);
  return 0;
}
template <typename T, class S>
int particles_tile_stats_impl(int nx, int ny, int nz, const T* sx, const T* sy, const T* sz, const double* inv_h, int bx, int by, int bz, int halo,
                              unsigned long long* out4) {
  EmuTileStatsOp<S> op;
  cic_walk_bricks(CicGrid{nx, ny, nz, {inv_h[0], inv_h[1], inv_h[2]}}, sx, sy, sz, bx, by, bz, halo, 1, op, &out4[3]);
  out4[0] = op.fallback; out4[1] = op.fallback_adds; out4[2] = op.flushed;
  return 0;
}

// the real type of the arrays chosen at run time, for the entry points with a scheme argument
template <class S>
int particles_paint_impl(int f64, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, int form, int bx, int by,
                         int bz, int halo, int nth, unsigned long long* A, unsigned long long* dropped) {
  return f64 ? particles_walk(nx, ny, nz, (const double*)sx, (const double*)sy, (const double*)sz, inv_h, form, bx, by, bz, halo, nth, EmuPaintOp<S>{A}, dropped)
             : particles_walk(nx, ny, nz, (const float*)sx, (const float*)sy, (const float*)sz, inv_h, form, bx, by, bz, halo, nth, EmuPaintOp<S>{A}, dropped);
}
template <class S>
int particles_tile_stats_any(int f64, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, int bx, int by, int bz,
                             int halo, unsigned long long* out4) {
  return f64 ? particles_tile_stats_impl<double, S>(nx, ny, nz, (const double*)sx, (const double*)sy, (const double*)sz, inv_h, bx, by, bz, halo, out4)
             : particles_tile_stats_impl<float, S>(nx, ny, nz, (const float*)sx, (const float*)sy, (const float*)sz, inv_h, bx, by, bz, halo, out4);
}
template <class S>
int particles_gather_impl(int f64, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, const void* W, void* G,
                          double coeff, int first, int form, int bx, int by, int bz, int halo, int nth, unsigned long long* dropped) {
  return f64 ? particles_walk(nx, ny, nz, (const double*)sx, (const double*)sy, (const double*)sz, inv_h, form, bx, by, bz, halo, nth,
                              EmuGatherOp<double, S>{(const double*)W, (double*)G, coeff, first}, dropped)
             : particles_walk(nx, ny, nz, (const float*)sx, (const float*)sy, (const float*)sz, inv_h, form, bx, by, bz, halo, nth,
                              EmuGatherOp<float, S>{(const float*)W, (float*)G, coeff, first}, dropped);
}

template <typename T>
int particles_accumulate_impl(int first, double coeff, const T* W, T* Q, long long n) {
  const T c = (T)coeff;
  for (long long i = 0; i < n; ++i) Q[i] = particles_axpy<T>(first != 0, c, W[i], first ? (T)0 : Q[i]);
  return 0;
}

template <typename T>
int generic_r2c_impl(int nx, int ny, int nz, const T* W, cplx<T>* K) {
  GenericDims d;
  if (!emu_dims<T>(nx, ny, nz, true, d)) return -1;
  const long long nzh = nz / 2 + 1;
  auto rx = make_twiddles<T>(nx), ry = make_twiddles<T>(ny), rz = make_twiddles<T>(nz);
  std::vector<cplx<T>> G((size_t)nx * ny * nzh), G2((size_t)nx * ny * nzh);
  EmuGenericOps<T> ops{rx.data(), ry.data(), rz.data(), nx, ny, nz, nz / 2, (long long)nx * ny, nullptr};
  ops.az = d.az;
  return generic_r2c_seq(ops, d, W, K, G.data(), G2.data());
}

template <typename T>
int generic_c2c_impl(int nx, int ny, int nz, int dir, cplx<T>* D) {
  GenericDims d;
  if (!emu_dims<T>(nx, ny, nz, false, d)) return -1;
  auto rx = make_twiddles<T>(nx), ry = make_twiddles<T>(ny), rz = make_twiddles<T>(nz);
  std::vector<cplx<T>> G((size_t)nx * ny * nz);
  EmuGenericOps<T> ops{rx.data(), ry.data(), rz.data(), nx, ny, nz, nz, (long long)nx * ny, nullptr};
  ops.az = d.az;
  return generic_c2c_seq(ops, d, D, G.data(), dir, dir > 0 ? 1.0 / ((double)nx * ny * nz) : 1.0);
}

// rf_realise_lognormal on an uploaded k-space array: x pass, the accumulating y pass (AccColIO: one Parseval partial per tile),
// sigma and the tables as lognormal_tables_kernel forms them, the z pass with the map in its epilogue (LognormalRowIO)
template <typename T>
int c2r_lognormal_impl(int nx, int ny, int nz, const cplx<T>* kspace, const double* growth, const double* density, cplx<T>* W,
                       double* sigma_out, double* s1, double* s2) {
  const long long nzc = nz / 2;
  const GenColIO<T> gio = gen_col_io<T>(W, x_geom(ny, nzc), kspace_params(nx, ny, nz), kspace, 0, (int)nzc);
  if (int rc = dispatch_col<T, +1, GenColIO<T>, GenSel>(nx, gio, (long long)ny * nzc)) return rc;
  // y pass with the accumulator (launch_col_plain_acc: whole columns): every "thread"'s sum is collected after its tile (the kernel's finish())
  double S = 0;
  auto collect = [&](long long, const std::vector<AccColIO<T>>& ios) {
    double a = 0;
    for (const auto& io : ios) a += io.weighted_sum();
    S += a;
  };
  if (int rc = dispatch_col<T, +1>(ny, acc_col_io<T>(W, y_geom(ny, nzc), nullptr, 0, (int)nzc), (long long)nx * nzc, collect)) return rc;
  const double n3 = (double)nx * ny * nz;
  double sigma = std::sqrt(S / ((double)nx * ny * n3 * n3));
  if (sizeof(T) == 4) sigma = (double)(float)sigma;
  std::vector<double> Ap(nz), Bp(nz);
  for (int z = 0; z < nz; ++z) {
    const double g = sigma * growth[z], t = g * g + 1.0;
    Ap[z] = std::sqrt(std::log(t)) / sigma * lognormal_ap_unit<T>(1.0 / n3);
    Bp[z] = (density ? density[z] : 1.0) / std::sqrt(t);
  }
  *sigma_out = sigma;
  return dispatch_row_c2r<T>((int)nzc, (long long)nx * ny, s1, s2, [&](auto c) {
    LognormalIO<T, decltype(c)::type::M> zio; zio.base = W; zio.scale = (T)(1.0 / n3); zio.M_of = (int)nzc; zio.Ap = Ap.data(); zio.Bp = Bp.data();
    return zio;
  });
}

// rf_realise_scaled_potential(factor_z) behind its generation pass, on an uploaded k-space array: x and y passes plain, the z pass with
// the per-z factor in its store (ScaleZRowIO), the row configuration from for_rows as launch_row_c2r_zscale takes it
template <typename T>
int c2r_zscale_impl(int nx, int ny, int nz, const cplx<T>* kspace, const double* factor_z, cplx<T>* W, double* s1, double* s2) {
  const long long nzc = nz / 2;
  const GenColIO<T> gio = gen_col_io<T>(W, x_geom(ny, nzc), kspace_params(nx, ny, nz), kspace, 0, (int)nzc);
  if (int rc = dispatch_col<T, +1, GenColIO<T>, GenSel>(nx, gio, (long long)ny * nzc)) return rc;
  if (int rc = plain_col_pass<T, +1>(ny, W, y_geom(ny, nzc), (long long)nx * nzc)) return rc;
  auto tw = make_twiddles<T>(2 * (int)nzc);
  return for_rows(sizeof(T) == 8, (int)nzc, -1, [&](auto r, auto c) {
    using C = typename decltype(c)::type;
    if constexpr (std::is_same<typename decltype(r)::type, T>::value) {
      ScaleZRowIO<T> io; io.base = W; io.scale = (T)(1.0 / ((double)nx * ny * nz)); io.M_of = (int)nzc; io.Sz = factor_z;
      run_row_c2r<C, ScaleZRowIO<T>>(io, (long long)nx * ny, tw.data(), s1, s2);
      return 0;
    } else {
      return -1;
    }
  });
}

// The loop behind emu_measure_power and emu_measure_multipoles (rf_core.h power_load / bin_cell over an array in array order, as the
// device sweep's cells).  g arrives cleared but for the estimator's own fields; edges: nbins + 1 edges in k, squared here as the host
// side of the device calls squares them.
template <typename P>
int measure_bins(int f64, int nx, int ny, int nz, int packed, const double* kx2, const double* ky2, const double* kz2, const void* S,
                 const double* edges, int nbins, P& g, unsigned long long* count, double* const (&sums)[BinSums<P>::N]) {
  constexpr int NS = BinSums<P>::N;
  if (nx < 1 || ny < 1 || nz < 2 || (nz & 1) || nbins < 1 || nbins > 1024 || !(kx2 && ky2 && kz2 && S && edges) || !(edges[0] >= 0.0)) return -1;
  for (int b = 0; b < nbins; ++b) if (!(edges[b] < edges[b + 1])) return -1;
  PowerParams& gp = bin_geom(g);
  gp.nx = nx; gp.ny = ny; gp.nz = nz; gp.nbins = nbins; gp.packed = packed != 0;
  gp.kx2 = kx2; gp.ky2 = ky2; gp.kz2 = kz2;
  std::vector<double> e2((size_t)nbins + 1);
  for (int b = 0; b <= nbins; ++b) e2[b] = edges[b] * edges[b];
  for (int b = 0; b < nbins; ++b) {
    count[b] = 0;
    for (int j = 0; j < NS; ++j) sums[j][b] = 0.0;
  }
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy)
      for (int iz = 0; iz <= nz / 2; ++iz) {
        int w = 0;
        double d[NS] = {};
        const int b = f64 ? bin_cell<double>(g, e2.data(), power_load<double>(gp, (const cplx<double>*)S, ix, iy, iz), ix, iy, iz, w, d)
                          : bin_cell<float>(g, e2.data(), power_load<float>(gp, (const cplx<float>*)S, ix, iy, iz), ix, iy, iz, w, d);
        if (b < 0) continue;
        count[b] += (unsigned long long)w;
        for (int j = 0; j < NS; ++j) sums[j][b] += d[j];
      }
  return 0;
}
}  // namespace

extern "C" {

// The row table of resident float32 deviates (rf_core.h make_rowloc / row_pair; mt_rowtab_kernel builds it on the device): where
// the generation pass finds the pair of cell kz of the row whose first stream cell is rows[i].  first = exclusive scan of the
// per-segment counts, nseg + 1 entries.  out[i * nzh + kz] = slot index in the runs; returns the "row spans more than two
// segments" flag.
int emu_row_lookup(const unsigned long long* first, int nseg, unsigned long long cap, unsigned nzh, const unsigned long long* rows, int n,
                   unsigned long long* out) {
  FastGenParams g;
  memset(&g, 0, sizeof g);
  std::vector<cplx<float>> dummy(1);
  g.noise32 = dummy.data(); g.seg_cap = cap;
  int bad = 0;
  for (int i = 0; i < n; ++i) {
    const RowLoc e = make_rowloc(first, nseg, rows[i], nzh, &bad);
    for (unsigned kz = 0; kz < nzh; ++kz) out[(size_t)i * nzh + kz] = (unsigned long long)(row_pair(g, e, (int)kz) - g.noise32);
  }
  return bad;
}

// the generic (any even shape) transforms: API-layout half spectrum <-> dense real field; c2c in place
int emu_generic_c2r(int f64, int nx, int ny, int nz, const void* K, void* W, double* s1, double* s2) {
  return f64 ? generic_c2r_impl<double>(nx, ny, nz, (const cplx<double>*)K, (double*)W, s1, s2)
             : generic_c2r_impl<float>(nx, ny, nz, (const cplx<float>*)K, (float*)W, s1, s2);
}
// emu_generate_kspace + emu_generic_c2r in one: the generation inside the x pass (honours emu_set_generic_threads / _tile / _cap)
int emu_generic_realise(int f64, int nx, int ny, int nz, const double* kx2, const double* ky2, const double* kz2,
                        const double* log10k, const double* sigma, int nt, int noise_mode, uint64_t seed,
                        const double* noise, void* W, double* s1, double* s2) {
  GenHost h;
  fill_gen(h, nx, ny, nz, kx2, ky2, kz2, log10k, sigma, nt, noise_mode, seed, noise);
  return f64 ? generic_c2r_from_impl<double>(nx, ny, nz, h.gp, nullptr, (double*)W, s1, s2)
             : generic_c2r_from_impl<float>(nx, ny, nz, h.gp, nullptr, (float*)W, s1, s2);
}
// K [nx][ny][nz/2+1] = i k_axis S (rf_core.h grad_cell over an array, as the elementwise derivative kernel): S has rows of spitch cells and
// holds delta(k) / k^2, or delta(k) with divide != 0 (kx2, ky2, kz2: the k^2 tables; S == K is allowed)
int emu_gradient_k(int f64, int nx, int ny, int nz, int axis, double scale, double dk, int divide, const double* kx2, const double* ky2,
                   const double* kz2, const void* S, long long spitch, void* K) {
  GradParams g;
  return emu_grad_params(nx, ny, nz, axis, scale, dk, divide, kx2, ky2, kz2, spitch, g) ? emu_deriv_k(f64, g, S, K) : -1;
}
// the field of that component with the factor applied inside the x pass (honours emu_set_generic_threads / _tile / _cap)
int emu_generic_gradient_c2r(int f64, int nx, int ny, int nz, int axis, double scale, double dk, int divide, const double* kx2, const double* ky2,
                             const double* kz2, const void* S, long long spitch, void* W, double* s1, double* s2) {
  GradParams g;
  return emu_grad_params(nx, ny, nz, axis, scale, dk, divide, kx2, ky2, kz2, spitch, g) ? emu_deriv_c2r(f64, g, S, W, s1, s2) : -1;
}
// K [nx][ny][nz/2+1] = D_a D_b S = -scale k_a k_b S (rf_core.h hess_cell over an array, as the elementwise derivative kernel), 0 <= a <= b <= 2;
// S, spitch, divide and S == K as emu_gradient_k
int emu_hessian_k(int f64, int nx, int ny, int nz, int a, int b, double scale, double dk_a, double dk_b, int divide, const double* kx2,
                  const double* ky2, const double* kz2, const void* S, long long spitch, void* K) {
  HessParams g;
  return emu_hess_params(nx, ny, nz, a, b, scale, dk_a, dk_b, divide, kx2, ky2, kz2, spitch, g) ? emu_deriv_k(f64, g, S, K) : -1;
}
// the field of that component with the factor applied inside the x pass (honours emu_set_generic_threads / _tile / _cap)
int emu_generic_hessian_c2r(int f64, int nx, int ny, int nz, int a, int b, double scale, double dk_a, double dk_b, int divide, const double* kx2,
                            const double* ky2, const double* kz2, const void* S, long long spitch, void* W, double* s1, double* s2) {
  HessParams g;
  return emu_hess_params(nx, ny, nz, a, b, scale, dk_a, dk_b, divide, kx2, ky2, kz2, spitch, g) ? emu_deriv_c2r(f64, g, S, W, s1, s2) : -1;
}
// one step (0 .. 4: FIRST, DIAG2, DIAG3, OFF, LAST) of the 2LPT source's sweep over n elements (rf_core.h lpt2_step, the function the
// kernel calls per element): H the component, T and S the accumulators; LAST leaves the source in H
int emu_lpt2_accumulate(int f64, int step, void* H, void* T, void* S, long long n) {
  if (n < 0 || !(H && T && S)) return -1;
  return f64 ? lpt2_accumulate_impl<double>(step, (double*)H, (double*)T, (double*)S, n)
             : lpt2_accumulate_impl<float>(step, (float*)H, (float*)T, (float*)S, n);
}
// The cloud-in-cell paint of the lattice particles displaced by (sx, sy, sz) -- dense [nx][ny][nz] arrays of float32 / float64 -- into the
// 64-bit grid A[nx][ny][nz] (cleared here; rf_core.h cic_particle, the functions rf_k_particles.hip calls).  form 1: every particle adds
// straight into A; form 2: bricks of bx x by x bz cells with a tile of brick + halo each, flushed with wrapped indices.  nth > 1: that many
// real host threads share A and the tile through atomic adds.  *dropped: particles with a non-finite displacement.
int emu_particles_paint_ex(int f64, int scheme, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, int form,
                           int bx, int by, int bz, int halo, int nth, unsigned long long* A, unsigned long long* dropped);
int emu_particles_paint(int f64, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, int form, int bx, int by,
                        int bz, int halo, int nth, unsigned long long* A, unsigned long long* dropped) {
  return emu_particles_paint_ex(f64, 2, nx, ny, nz, sx, sy, sz, inv_h, form, bx, by, bz, halo, nth, A, dropped);
}
// the same with the assignment scheme: 2 cloud in cell, 3 triangular-shaped cloud (rf_core.h tsc_particle, 27 cells under the same walks)
int emu_particles_paint_ex(int f64, int scheme, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, int form,
                           int bx, int by, int bz, int halo, int nth, unsigned long long* A, unsigned long long* dropped) {
  if (scheme != 2 && scheme != 3) return -1;
  if (nx < 1 || ny < 1 || nz < 1 || !(sx && sy && sz && inv_h && A && dropped) || (form != 1 && form != 2) || nth < 1 || nth > 1024) return -1;
  if (form == 2 && (bx < 1 || by < 1 || bz < 1 || halo < 1)) return -1;
  memset(A, 0, (size_t)nx * ny * nz * 8);
  return scheme == 3 ? particles_paint_impl<EmuTsc>(f64, nx, ny, nz, sx, sy, sz, inv_h, form, bx, by, bz, halo, nth, A, dropped)
                     : particles_paint_impl<EmuCic>(f64, nx, ny, nz, sx, sy, sz, inv_h, form, bx, by, bz, halo, nth, A, dropped);
}
// the same with the half-cell shift as an argument (rf_particles_paint_shifted): half_cell = 0 is emu_particles_paint_ex, 1 paints the
// particles at u + 1/2 on every axis (rf_core.h cic_axis_half), anything else is refused
int emu_particles_paint_shifted(int f64, int scheme, int half_cell, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz,
                                const double* inv_h, int form, int bx, int by, int bz, int halo, int nth, unsigned long long* A, unsigned long long* dropped) {
  if (half_cell == 0) return emu_particles_paint_ex(f64, scheme, nx, ny, nz, sx, sy, sz, inv_h, form, bx, by, bz, halo, nth, A, dropped);
  if (half_cell != 1 || (scheme != 2 && scheme != 3)) return -1;
  if (nx < 1 || ny < 1 || nz < 1 || !(sx && sy && sz && inv_h && A && dropped) || (form != 1 && form != 2) || nth < 1 || nth > 1024) return -1;
  if (form == 2 && (bx < 1 || by < 1 || bz < 1 || halo < 1)) return -1;
  memset(A, 0, (size_t)nx * ny * nz * 8);
  return scheme == 3 ? particles_paint_impl<EmuTscHalf>(f64, nx, ny, nz, sx, sy, sz, inv_h, form, bx, by, bz, halo, nth, A, dropped)
                     : particles_paint_impl<EmuCicHalf>(f64, nx, ny, nz, sx, sy, sz, inv_h, form, bx, by, bz, halo, nth, A, dropped);
}
// The interlacing combine K <- (S + p K) / 2 over two half spectra [nx][ny][nz/2 + 1] (rf_core.h interlace_mul / interlace_cell, the
// functions interlace_kernel calls per cell): px, py, pz are nx, ny, nz/2 + 1 interleaved (re, im) float64 pairs, null = all ones
int emu_kspace_interlace(int f64, int nx, int ny, int nz, const void* S, void* K, const double* px, const double* py, const double* pz) {
  if (nx < 1 || ny < 1 || nz < 2 || (nz & 1) || !(S && K) || S == K) return -1;
  const int nzh = nz / 2 + 1;
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy) {
      const double xr = px ? px[2 * ix] : 1.0, xi = px ? px[2 * ix + 1] : 0.0, yr = py ? py[2 * iy] : 1.0, yi = py ? py[2 * iy + 1] : 0.0;
      double ar, ai;
      interlace_mul(xr, xi, yr, yi, ar, ai);
      const long long row = ((long long)ix * ny + iy) * nzh;
      for (int iz = 0; iz < nzh; ++iz) {
        const double zr = pz ? pz[2 * iz] : 1.0, zi = pz ? pz[2 * iz + 1] : 0.0;
        if (f64) ((cplx<double>*)K)[row + iz] = interlace_cell<double>(((const cplx<double>*)S)[row + iz], ((cplx<double>*)K)[row + iz], ar, ai, zr, zi);
        else ((cplx<float>*)K)[row + iz] = interlace_cell<float>(((const cplx<float>*)S)[row + iz], ((cplx<float>*)K)[row + iz], ar, ai, zr, zi);
      }
    }
  return 0;
}
// the tiled form's traffic for these particles, by the kernel's own rule: out4 = {particles that leave their brick's tile, their adds
// straight into A, non-zero tile cells flushed, dropped particles}
int emu_particles_tile_stats_ex(int f64, int scheme, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, int bx,
                                int by, int bz, int halo, unsigned long long* out4);
int emu_particles_tile_stats(int f64, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, int bx, int by, int bz,
                             int halo, unsigned long long* out4) {
  return emu_particles_tile_stats_ex(f64, 2, nx, ny, nz, sx, sy, sz, inv_h, bx, by, bz, halo, out4);
}
// the same with the assignment scheme (2, 3): the triangular-shaped cloud's 27 adds per particle and its tighter tile rule
int emu_particles_tile_stats_ex(int f64, int scheme, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, int bx,
                                int by, int bz, int halo, unsigned long long* out4) {
  if (scheme != 2 && scheme != 3) return -1;
  if (nx < 1 || ny < 1 || nz < 1 || !(sx && sy && sz && inv_h && out4) || bx < 1 || by < 1 || bz < 1 || halo < 1) return -1;
  return scheme == 3 ? particles_tile_stats_any<EmuTsc>(f64, nx, ny, nz, sx, sy, sz, inv_h, bx, by, bz, halo, out4)
                     : particles_tile_stats_any<EmuCic>(f64, nx, ny, nz, sx, sy, sz, inv_h, bx, by, bz, halo, out4);
}
// The cloud-in-cell gather of the dense real field W at the lattice particles displaced by (sx, sy, sz) into G[nx][ny][nz], indexed by
// the particle's lattice cell (rf_core.h cic_gather_value, the functions rf_k_particles.hip calls): G = (T)(coeff g) (first) or
// (T)((double)G + coeff g).  form 1: every particle loads its eight cells from W; form 2: bricks of bx x by x bz cells whose tile of W
// (brick + halo) is really staged in an array and read there.  nth real host threads.  *dropped: particles with a non-finite
// displacement (they gather 0).
int emu_particles_gather_ex(int f64, int scheme, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h,
                            const void* W, void* G, double coeff, int first, int form, int bx, int by, int bz, int halo, int nth,
                            unsigned long long* dropped);
int emu_particles_gather(int f64, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h, const void* W, void* G,
                         double coeff, int first, int form, int bx, int by, int bz, int halo, int nth, unsigned long long* dropped) {
  return emu_particles_gather_ex(f64, 2, nx, ny, nz, sx, sy, sz, inv_h, W, G, coeff, first, form, bx, by, bz, halo, nth, dropped);
}
// the same with the assignment scheme (2, 3): rf_core.h tsc_gather_cells, 27 values per particle reduced three at a time
int emu_particles_gather_ex(int f64, int scheme, int nx, int ny, int nz, const void* sx, const void* sy, const void* sz, const double* inv_h,
                            const void* W, void* G, double coeff, int first, int form, int bx, int by, int bz, int halo, int nth,
                            unsigned long long* dropped) {
  if (scheme != 2 && scheme != 3) return -1;
  if (nx < 1 || ny < 1 || nz < 1 || !(sx && sy && sz && inv_h && W && G && dropped) || (form != 1 && form != 2) || nth < 1 || nth > 1024) return -1;
  if (form == 2 && (bx < 1 || by < 1 || bz < 1 || halo < 1)) return -1;
  return scheme == 3 ? particles_gather_impl<EmuTsc>(f64, nx, ny, nz, sx, sy, sz, inv_h, W, G, coeff, first, form, bx, by, bz, halo, nth, dropped)
                     : particles_gather_impl<EmuCic>(f64, nx, ny, nz, sx, sy, sz, inv_h, W, G, coeff, first, form, bx, by, bz, halo, nth, dropped);
}
// Q = coeff W (first) or Q + coeff W over n elements (rf_core.h particles_axpy, the function the kernel calls per element)
int emu_particles_accumulate(int f64, int first, double coeff, const void* W, void* Q, long long n) {
  if (n < 0 || !(W && Q)) return -1;
  return f64 ? particles_accumulate_impl<double>(first, coeff, (const double*)W, (double*)Q, n)
             : particles_accumulate_impl<float>(first, coeff, (const float*)W, (float*)Q, n);
}
// W = (double)A 2^-48 - 1 rounded once (rf_core.h cic_delta)
int emu_particles_delta(int f64, const unsigned long long* A, void* W, long long n) {
  if (n < 0 || !(A && W)) return -1;
  for (long long i = 0; i < n; ++i) {
    if (f64) ((double*)W)[i] = cic_delta<double>(A[i]); else ((float*)W)[i] = cic_delta<float>(A[i]);
  }
  return 0;
}
// the binned power spectrum (measure_bins with rf_core.h power_cell, as rf_measure_power's sweep): S is the API-layout half spectrum
// [nx][ny][nz/2+1], or with packed != 0 the array [nx][ny][nz/2] the tiled forward passes leave (slot kz = 0 = A0 + i A_nyq)
int emu_measure_power(int f64, int nx, int ny, int nz, int packed, const double* kx2, const double* ky2, const double* kz2, const void* S,
                      const double* edges, int nbins, unsigned long long* count, double* sum_k, double* sum_p) {
  PowerParams g;
  memset(&g, 0, sizeof(g));
  double* const sums[2] = {sum_k, sum_p};
  return measure_bins(f64, nx, ny, nz, packed, kx2, ky2, kz2, S, edges, nbins, g, count, sums);
}
// the power spectrum multipoles (measure_bins with multipole_cell, as rf_measure_multipoles' sweep): S, packed and edges as
// emu_measure_power's; los 0, 1, 2; cx, cy, cz: tables of nx, ny, nz/2 + 1 finite positive entries, or null
int emu_measure_multipoles(int f64, int nx, int ny, int nz, int packed, int los, const double* kx2, const double* ky2, const double* kz2,
                           const void* S, const double* edges, int nbins, const double* cx, const double* cy, const double* cz,
                           unsigned long long* count, double* sum_k, double* m0, double* m2, double* m4) {
  if (los < 0 || los > 2 || !(count && sum_k && m0 && m2 && m4)) return -1;
  const double* comp[3] = {cx, cy, cz};
  const int clen[3] = {nx, ny, nz / 2 + 1};
  for (int a = 0; a < 3; ++a)
    for (int i = 0; comp[a] && i < clen[a]; ++i) if (!(std::isfinite(comp[a][i]) && comp[a][i] > 0.0)) return -1;
  MultipoleParams g;
  memset(&g, 0, sizeof(g));
  g.los = los; g.cx = cx; g.cy = cy; g.cz = cz;
  double* const sums[4] = {sum_k, m0, m2, m4};
  return measure_bins(f64, nx, ny, nz, packed, kx2, ky2, kz2, S, edges, nbins, g, count, sums);
}
// The shell filter of rf_measure_bispectrum (rf_core.h shell_cell, the function shell_filter_kernel calls per cell): M = the API-layout
// half spectrum K restricted to shell `shell` of the nbins + 1 edges (squared here as the host side of the device call squares them);
// ax, ay, az: tables of nx, ny, nz/2 + 1 finite positive entries or null; unit != 0: 1 inside the shell, the tables ignored
int emu_kspace_shell(int f64, int nx, int ny, int nz, const double* kx2, const double* ky2, const double* kz2, const void* K, const double* edges,
                     int nbins, int shell, const double* ax, const double* ay, const double* az, int unit, void* M) {
  if (nx < 1 || ny < 1 || nz < 2 || (nz & 1) || nbins < 1 || nbins > BISPECTRUM_MAX_BINS || shell < 0 || shell >= nbins ||
      !(kx2 && ky2 && kz2 && K && M && edges) || K == M || !(edges[0] >= 0.0))
    return -1;
  for (int b = 0; b < nbins; ++b) if (!(edges[b] < edges[b + 1])) return -1;
  const double* amp[3] = {ax, ay, az};
  const int alen[3] = {nx, ny, nz / 2 + 1};
  for (int a = 0; a < 3 && !unit; ++a)
    for (int i = 0; amp[a] && i < alen[a]; ++i) if (!(std::isfinite(amp[a][i]) && amp[a][i] > 0.0)) return -1;
  ShellParams g;
  memset(&g, 0, sizeof(g));
  g.p.nx = nx; g.p.ny = ny; g.p.nz = nz; g.p.nbins = nbins;
  g.p.kx2 = kx2; g.p.ky2 = ky2; g.p.kz2 = kz2;
  g.unit = unit != 0;
  if (!unit) { g.ax = ax; g.ay = ay; g.az = az; }
  std::vector<double> e2((size_t)nbins + 1);
  for (int b = 0; b <= nbins; ++b) e2[b] = edges[b] * edges[b];
  const int nzh = nz / 2 + 1;
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy) {
      const long long row = ((long long)ix * ny + iy) * nzh;
      for (int iz = 0; iz < nzh; ++iz) {
        if (f64) ((cplx<double>*)M)[row + iz] = shell_cell<double>(g, e2.data(), shell, ((const cplx<double>*)K)[row + iz], ix, iy, iz);
        else ((cplx<float>*)M)[row + iz] = shell_cell<float>(g, e2.data(), shell, ((const cplx<float>*)K)[row + iz], ix, iy, iz);
      }
    }
  return 0;
}
// The triple sums of rf_measure_bispectrum over nbins dense fields F[nbins][ncells] of the plan's real type (rf_core.h bispectrum_add,
// the function bispectrum_sum_kernel calls per term): out[t] = sum over the cells, in cell order, of D_b1 D_b2 D_b3 for the ntriples
// triples (b1, b2, b3), 0 <= b1 <= b2 <= b3 < nbins.  The device sums the same terms in its own fixed order.
int emu_bispectrum_sums(int f64, long long ncells, int nbins, const void* F, const int* triples, int ntriples, double* out) {
  if (ncells < 1 || nbins < 1 || nbins > BISPECTRUM_MAX_BINS || ntriples < 1 || ntriples > BISPECTRUM_MAX_TRIPLES || !(F && triples && out)) return -1;
  for (int t = 0; t < ntriples; ++t)
    if (!(0 <= triples[3 * t] && triples[3 * t] <= triples[3 * t + 1] && triples[3 * t + 1] <= triples[3 * t + 2] && triples[3 * t + 2] < nbins)) return -1;
  for (int t = 0; t < ntriples; ++t) {
    const long long o1 = triples[3 * t] * ncells, o2 = triples[3 * t + 1] * ncells, o3 = triples[3 * t + 2] * ncells;
    double s = 0.0;
    for (long long i = 0; i < ncells; ++i) {
      if (f64) s = bispectrum_add(s, ((const double*)F)[o1 + i], ((const double*)F)[o2 + i], ((const double*)F)[o3 + i]);
      else s = bispectrum_add(s, (double)((const float*)F)[o1 + i], (double)((const float*)F)[o2 + i], (double)((const float*)F)[o3 + i]);
    }
    out[t] = s;
  }
  return 0;
}
int emu_generic_r2c(int f64, int nx, int ny, int nz, const void* W, void* K) {
  return f64 ? generic_r2c_impl<double>(nx, ny, nz, (const double*)W, (cplx<double>*)K)
             : generic_r2c_impl<float>(nx, ny, nz, (const float*)W, (cplx<float>*)K);
}
int emu_generic_c2c(int f64, int nx, int ny, int nz, int dir, void* D) {
  return f64 ? generic_c2c_impl<double>(nx, ny, nz, dir, (cplx<double>*)D) : generic_c2c_impl<float>(nx, ny, nz, dir, (cplx<float>*)D);
}

int emu_c2r_lognormal(int f64, int nx, int ny, int nz, const void* kspace, const double* growth, const double* density, void* W,
                      double* sigma_out, double* s1, double* s2) {
  return f64 ? c2r_lognormal_impl<double>(nx, ny, nz, (const cplx<double>*)kspace, growth, density, (cplx<double>*)W, sigma_out, s1, s2)
             : c2r_lognormal_impl<float>(nx, ny, nz, (const cplx<float>*)kspace, growth, density, (cplx<float>*)W, sigma_out, s1, s2);
}

int emu_c2r_zscale(int f64, int nx, int ny, int nz, const void* kspace, const double* factor_z, void* W, double* s1, double* s2) {
  return f64 ? c2r_zscale_impl<double>(nx, ny, nz, (const cplx<double>*)kspace, factor_z, (cplx<double>*)W, s1, s2)
             : c2r_zscale_impl<float>(nx, ny, nz, (const cplx<float>*)kspace, factor_z, (cplx<float>*)W, s1, s2);
}
// exp_scaled64 by itself on n arguments (units of ln2 / 64).  stride 1: on rf_exp2_tab, as LognormalRowIO<double, 0> reads it; stride 18
// (LognormalRowIO<double, 1>::ESTRIDE): on the copy that IO's own stage() leaves in the pad slots of a tile of rows of 512 complex128,
// every other double of that tile NaN
int emu_exp_scaled64(const double* t, double* out, long long n, int stride) {
  using IO = LognormalRowIO<double, 1>;
  if (stride == 1) {
    for (long long i = 0; i < n; ++i) out[i] = exp_scaled64<1>(t[i], rf_exp2_tab);
    return 0;
  }
  if (stride != IO::ESTRIDE) return -1;
  using C = RowSel<double, 512>::type;
  std::vector<double> lds((size_t)C::LDS_BYTES / sizeof(double), std::nan(""));
  IO io{};
  for (int tid = 0; tid < C::NT; ++tid) io.stage<C>(tid, lds.data());
  for (long long i = 0; i < n; ++i) out[i] = exp_scaled64<IO::ESTRIDE>(t[i], io.etab);
  return 0;
}

// fused realisation with the fast native generation (float32 arithmetic; f64 != 0: float64 plan, values widened);
// [xlo, xhi] = log10 k range of the grid (padded)
// emu_realise_fast_ex: the same with everything launch_col_fastgen is told (FastCall above) -- pot 0 / 1 / 2 with pscale; src 0 / 1
// (noise64: float64 deviates in the API layout) / 2 (noise32: float32 pairs in the replay's runs of `cap` slots per segment, first:
// exclusive scan of the per-segment counts, nseg + 1 entries); rows [x0, x1) and planes [kz0, kz0 + nzl) (nzl < 0: all).  W is the
// whole grid's buffer: a call with finish = 0 runs its x pass into it and returns, the last call (finish != 0) also runs the y and z
// passes, so the ranks of a job are one call each; finish = 2: no transform at all -- W receives the packed cells the pass loads
// (fast_loads: [nx][ny][nzl] complex, the kz = 0 slot repaired), the pass's own k-space values.  P (pot = 1): the call's potential array [nx][ny][ppitch], ppitch as
// rf_plan_create sets it (nzl + 1 cells, padded to nzl + 2 or nzl + 64 on float32 plans), rows of its own planes + the Nyquist plane.
int emu_realise_fast_ex(int f64, int nx, int ny, int nz, const double* kx2, const double* ky2, const double* kz2,
                        const double* log10k, const double* sigma, int nt, uint64_t seed, double xlo, double xhi, double dkx,
                        int pot, double pscale, int src, const double* noise64, const void* noise32, const unsigned long long* first, int nseg,
                        unsigned long long cap, int x0, int x1, int kz0, int nzl, int finish, void* W, void* P, double* s1, double* s2) {
  GenHost h;
  fill_gen(h, nx, ny, nz, kx2, ky2, kz2, log10k, sigma, nt, 0, seed, nullptr);
  FastCall c;
  c.pot = pot; c.pscale = pscale; c.src = src; c.noise64 = noise64; c.noise32 = (const cplx<float>*)noise32; c.first = first; c.nseg = nseg; c.cap = cap;
  c.x0 = x0; c.x1 = x1; c.kz0 = kz0; c.nzl = nzl; c.loads = finish == 2;
  return f64 ? realise_fast_impl<double>(nx, ny, nz, h, seed, xlo, xhi, dkx, c, finish != 0, (cplx<double>*)W, (cplx<double>*)P, s1, s2)
             : realise_fast_impl<float>(nx, ny, nz, h, seed, xlo, xhi, dkx, c, finish != 0, (cplx<float>*)W, (cplx<float>*)P, s1, s2);
}
int emu_realise_fast(int f64, int nx, int ny, int nz, const double* kx2, const double* ky2, const double* kz2,
                     const double* log10k, const double* sigma, int nt, uint64_t seed, double xlo, double xhi,
                     double dkx, void* W, double* s1, double* s2) {
  return emu_realise_fast_ex(f64, nx, ny, nz, kx2, ky2, kz2, log10k, sigma, nt, seed, xlo, xhi, dkx, 0, 1.0, 0, nullptr, nullptr, nullptr, 0, 0,
                             0, 1 << 30, 0, -1, 1, W, nullptr, s1, s2);
}
// rf_select.h fastgen_variant as five numbers (valid, slab, pot, src, halves); col_replicate_supported
int emu_fastgen_variant(int f64, int N, int emit, int n64, int n32, int pot, int slab, int* out5) {
  const FastVariant v = fastgen_variant(f64, N, emit != 0, n64 != 0, n32 != 0, pot != 0, slab != 0);
  const int r[5] = {v.valid, v.slab, v.pot, v.src, v.halves};
  std::copy(r, r + 5, out5);
  return v.valid;
}
int emu_col_replicate_supported(int f64, int N, int nranks) { return col_replicate_supported(f64, N, nranks); }

// Row T alone: the fast float32 sigma(|k|^2) lookup (per-bin records, rf_core.h fast_sigma) next to the exact float64
// interpolation of the same table, for n values of |k|^2 -- bounds the table-lookup error separately from the
// transcendental error of the deviates.  [xlo, xhi] = padded log10 k range of the grid, as the library passes it.
int emu_fast_sigma(const double* log10k, const double* sigma, int nt, double xlo, double xhi, const float* k2, int n,
                   float* out_fast, double* out_exact) {
  SigmaTableHost tab;
  build_sigma_table(log10k, sigma, nt, tab);
  std::vector<FastRec> rec;
  double x0, dx;
  if (!build_fast_records(tab, xlo, xhi, rec, x0, dx)) return -3;
  FastGenParams f;
  memset(&f, 0, sizeof f);
  f.rec = rec.data(); f.nbins = (int)rec.size();
  f.u_scale = (float)(0.5 * std::log10(2.0) / dx); f.u_off = (float)(-x0 / dx);
  GenParams g;
  memset(&g, 0, sizeof g);
  g.xt = tab.xt.data(); g.st = tab.st.data(); g.sl = tab.sl.data(); g.bin = tab.bin.data();
  g.nt = nt; g.nbins = (int)tab.bin.size(); g.x0 = tab.x0; g.inv_dx = tab.inv_dx;
  for (int i = 0; i < n; ++i) {
    out_fast[i] = fast_sigma(f, rec.data(), k2[i]);
    out_exact[i] = sigma_lookup(g, 0.5 * std::log10((double)k2[i]));
  }
  return f.nbins;
}

// k-space after symmetrise in the API layout [nx][ny][nz/2+1] (rows K,T,R,S)
int emu_generate_kspace(int f64, int nx, int ny, int nz, const double* kx2, const double* ky2, const double* kz2,
                        const double* log10k, const double* sigma, int nt, int noise_mode, uint64_t seed,
                        const double* noise, void* out) {
  GenHost h;
  fill_gen(h, nx, ny, nz, kx2, ky2, kz2, log10k, sigma, nt, noise_mode, seed, noise);
  const int nzh = nz / 2 + 1;
  for (int ix = 0; ix < nx; ++ix)
    for (int iy = 0; iy < ny; ++iy)
      for (int iz = 0; iz < nzh; ++iz) {
        const size_t c = ((size_t)ix * ny + iy) * nzh + iz;
        if (f64) ((cplx<double>*)out)[c] = gen_cell<double>(h.gp, seed, ix, iy, iz);
        else     ((cplx<float>*)out)[c] = gen_cell<float>(h.gp, seed, ix, iy, iz);
      }
  return 0;
}

// the gathering z pass alone: X = blocked intermediate [nx / rb][M / tc][ny][rb][tc] -> W dense real rows [nx][ny][2 M]
int emu_row_c2r_xgather(int f64, int M, int nx, int ny, int tc, int rb, const void* X, void* W, double scale, double* s1, double* s2) {
  if (!row_c2r_xgather_ok(f64, M, tc, rb) || nx % rb) return -2;
  return with_real(f64, [&](auto r) {
    using R = decltype(r);
    return xgather_row_c2r<typename R::type>(M, nx, ny, tc, rb, R::p(X), R::p(W), scale, s1, s2);
  });
}

// 1: c2r transforms hand x -> y through the blocked intermediate where the library would (rf_select.h xpose_shape_ok); 0 (default): in place
int emu_set_xposed(int on) { const int old = g_xposed; g_xposed = on; return old; }
int emu_set_rowblock(int rb) { const int old = g_rowblock; g_rowblock = rb; return old; }
// the longest line the generic path keeps whole (0 = the library's cap, 8192 complex64 / 4096 complex128): longer axes take the four-step
// form -- lowered by tests so that small grids exercise it
int emu_set_generic_cap(int cap) { const int old = g_generic_cap; g_generic_cap = cap; return old; }
// 1 (default): strided lines that fit the cap but prefer the four-step form run it, as the library decides (rf_generic.h
// generic_axis_form); 0: every axis that fits is one line.  Returns the old value.
int emu_set_generic_prefer_split(int on) { const int old = g_generic_prefer_split; g_generic_prefer_split = on ? 1 : 0; return old; }
// The form an axis of length n runs in (strided: an x or y axis; else the contiguous one) under the emulator's cap and switch -- with
// their defaults, the library's: out32 as emu_form_out.  Returns 1, or 0 where the axis is not served.
int emu_generic_axis_form(int f64, long long n, int strided, int* out32) {
  const int cap = g_generic_cap > 0 ? g_generic_cap : generic_max_axis(f64), es = f64 ? 16 : 8;
  GenericAxis ax;
  GenericLong lg;
  if (!generic_axis_form(n, cap, es, strided != 0, ax, lg, g_generic_prefer_split != 0)) return 0;
  emu_form_out(ax, lg, es, out32);
  return 1;
}
// ... and of the three axes of a packed (the contiguous axis at nz / 2) or c2c shape: out96 = x, y, z.  0: the emulator refuses the shape
int emu_generic_shape_form(int f64, int nx, int ny, int nz, int packed, int* out96) {
  GenericDims d;
  if (nx < 1 || ny < 1 || nz < 1 || !(f64 ? emu_dims<double>(nx, ny, nz, packed != 0, d) : emu_dims<float>(nx, ny, nz, packed != 0, d))) return 0;
  const int es = f64 ? 16 : 8;
  emu_form_out(d.ax, d.lx, es, out96);
  emu_form_out(d.ay, d.ly, es, out96 + 32);
  emu_form_out(d.az, d.lz, es, out96 + 64);
  return 1;
}
int emu_set_generic_tile(int tc) { const int old = g_generic_tile; g_generic_tile = tc > 0 ? tc : 3; return old; }
// host threads per block of the generic path (1, the default: one "thread" with a no-op barrier).  With nth > 1 the block functions
// run on nth threads with a real barrier; nth a multiple of the tile takes the kernels' own walk (GenericWalk::fixed)
int emu_set_generic_threads(int nth) { const int old = g_generic_threads; g_generic_threads = nth > 1 ? (nth < 1024 ? nth : 1024) : 1; return old; }
// 1 (default): the float32 generation pass of length 1024 on tile pairs (ColPair), as the library; 0: one tile per workgroup (ColFFT)
int emu_set_pairs(int on) { const int old = g_pairs; g_pairs = on; return old; }
// 1 (default): in-place strided passes take the halves form (Col2) where launch_col_plain does; 0: whole columns everywhere
int emu_set_col_halves(int on) { const int old = g_col_halves; g_col_halves = on; return old; }
// The launches of a fast generation pass as five numbers per step (kind, io, count, mul, skip_period: rf_select.h FastStep), at most
// `max` steps; returns their number.  emu_fast_steps: what the last emu_realise_fast ran; emu_fast_visits: how often that call
// transformed each tile of the x pass (out[tile], at most `max` tiles; returns the number of tiles); emu_fastgen_sequence: rf_select.h
// fastgen_sequence called directly for the pass of that grid (honours emu_set_xposed / _rowblock / _pairs), -2 where the library refuses
static int copy_steps(const FastStep* st, int n, long long* out5, int max) {
  for (int i = 0; i < n && i < max; ++i) {
    const long long v[5] = {st[i].kind, st[i].io, st[i].count, st[i].mul, st[i].skip_period};
    std::copy(v, v + 5, out5 + 5 * i);
  }
  return n;
}
int emu_fast_steps(long long* out5, int max) { return copy_steps(g_fast_steps.data(), (int)g_fast_steps.size(), out5, max); }
long long emu_fast_visits(int* out, long long max) {
  std::copy(g_fast_visits.begin(), g_fast_visits.begin() + std::min<long long>(max, (long long)g_fast_visits.size()), out);
  return (long long)g_fast_visits.size();
}
// emu_fastgen_sequence_ex: of the variant the flags select (emit, n64, n32, pot as emu_fastgen_variant), rows [x0, x1) and planes
// [kz0, kz0 + nzl) (nzl < 0: all) -- a kz-slab rank's pass runs on the geometry of its own planes
int emu_fastgen_sequence_ex(int f64, int nx, int ny, int nz, int emit, int n64, int n32, int pot, int x0, int x1, int kz0, int nzl, long long* out5, int max) {
  return with_real(f64, [&](auto r) {
    using T = typename decltype(r)::type;
    const long long nzc = nz / 2, nl = nzl < 0 ? nzc : nzl;
    FastCall c;
    c.pot = emit ? 2 : pot ? 1 : 0; c.src = n64 ? 1 : n32 ? 2 : 0; c.x0 = x0; c.x1 = x1; c.kz0 = kz0; c.nzl = (int)nl;
    const bool whole = kz0 == 0 && nl == nzc && !c.slab(nx);
    const ColGeom g = whole && xposed<T>(nx, ny, nzc) ? xposed_x_geom<T>(nx, ny, nzc) : x_geom(ny, nl);
    return with_fast_pass<T>(nx, g, (long long)ny * nl, (int)nl, c, [&](auto, const FastSequence& q) { return copy_steps(q.step, q.n, out5, max); });
  });
}
int emu_fastgen_sequence(int f64, int nx, int ny, int nz, long long* out5, int max) {
  return emu_fastgen_sequence_ex(f64, nx, ny, nz, 0, 0, 0, 0, 0, 1 << 30, 0, -1, out5, max);
}
// FastGenColIOT::share_row (rf_fft_gen.h): the butterfly row of slot jl when L butterflies are dealt to slots of S per wave so that
// the rows +-ix sit 32 lanes apart (the sigma exchange of the x pass); a host-side table for the bijection test
// (xs2_phase < 0: the whole-column form XS = 1; 0 / 1: the even / odd phase of the two-half-transform form XS = 2)
int emu_share_row(int jl, int L, int S, int xs2_phase) {
  if (xs2_phase < 0) { FastGenColIOT<0> io; return io.share_row(jl, L, S); }
  FastGenColIOT<0, 0, 0, 0, 2> io;
  io.set_phase(xs2_phase);
  return io.share_row(jl, L, S);
}
// generic_pos (rf_generic.h): where element e of a line of n goes in the LDS image of the in-place transform; out[e] = position,
// returns 1 when the axis is smooth (radices 2..5), 0 when the positions are the identity (two-buffer form), -1 when n does not factor
int emu_generic_positions(int n, int* out) {
  GenericAxis ax;
  if (!generic_factor(n, ax)) return -1;
  for (int e = 0; e < n; ++e) out[e] = generic_pos(ax, e);
  return generic_smooth(ax) ? 1 : 0;
}
// FastDiv (rf_generic.h): the first a < amax at which a / d or a % d by multiply-high differs from the machine's division; -1 if none
long long emu_fastdiv_first_error(unsigned d, unsigned amax) {
  const FastDiv fd(d, generic_magic(d));
  const FastDiv fd2(d);
  for (unsigned a = 0; a < amax; ++a) {
    uint32_t q, r;
    fd.divmod(a, q, r);
    if (q != a / d || r != a % d || fd2.div(a) != a / d) return (long long)a;
  }
  return -1;
}
int emu_xpose_applies(int f64, int nx, int ny, int nz) { return f64 ? xposed<double>(nx, ny, nz / 2) : xposed<float>(nx, ny, nz / 2); }

// full fused realisation: generation + x, y, z passes -> W (real [nx][ny][nz]) and (sum, sumsq)
int emu_realise(int f64, int nx, int ny, int nz, const double* kx2, const double* ky2, const double* kz2,
                const double* log10k, const double* sigma, int nt, int noise_mode, uint64_t seed,
                const double* noise, void* W, double* s1, double* s2) {
  GenHost h;
  fill_gen(h, nx, ny, nz, kx2, ky2, kz2, log10k, sigma, nt, noise_mode, seed, noise);
  return f64 ? c2r_impl<double>(nx, ny, nz, &h, nullptr, (cplx<double>*)W, s1, s2)
             : c2r_impl<float>(nx, ny, nz, &h, nullptr, (cplx<float>*)W, s1, s2);
}

// unfused c2r of an API-layout k-space array
int emu_c2r(int f64, int nx, int ny, int nz, const void* kspace, void* W, double* s1, double* s2) {
  return f64 ? c2r_impl<double>(nx, ny, nz, nullptr, (const cplx<double>*)kspace, (cplx<double>*)W, s1, s2)
             : c2r_impl<float>(nx, ny, nz, nullptr, (const cplx<float>*)kspace, (cplx<float>*)W, s1, s2);
}

// forward r2c of a dense real field [nx][ny][nz] into the API k layout [nx][ny][nz/2+1]
int emu_r2c(int f64, int nx, int ny, int nz, const void* field, void* K) {
  return f64 ? r2c_impl<double>(nx, ny, nz, (const double*)field, (cplx<double>*)K)
             : r2c_impl<float>(nx, ny, nz, (const float*)field, (cplx<float>*)K);
}

// unpacked complex-to-complex transform in place: dir = +1 inverse (1/N), -1 forward
int emu_c2c(int f64, int nx, int ny, int nz, int dir, void* data) {
  if (f64) return dir > 0 ? c2c_impl<double, +1>(nx, ny, nz, (cplx<double>*)data) : c2c_impl<double, -1>(nx, ny, nz, (cplx<double>*)data);
  return dir > 0 ? c2c_impl<float, +1>(nx, ny, nz, (cplx<float>*)data) : c2c_impl<float, -1>(nx, ny, nz, (cplx<float>*)data);
}

// one strided FFT pass over data[(C / inner) * outer_stride + C % inner + row * row_stride]: the whole-column configuration of length N
// (the per-length test of ColFFT; the library keeps these kernels at 1024 / 2048 float32 for geometries the halves do not fit)
int emu_col_fft(int f64, int N, int dir, void* data, long long ncols, long long inner, long long outer_stride,
                long long row_stride) {
  const ColGeom g{inner, outer_stride, row_stride};
  return with_real(f64, [&](auto r) {
    using R = decltype(r); using T = typename R::type;
    PlainColIO<T> io; io.base = R::p(data); io.g = g;
    return with_dir(dir, [&](auto d) { return dispatch_col<T, decltype(d)::value>(N, io, ncols); });
  });
}

}  // extern "C"
