// rf_select.h -- which kernel variant a tiled pass takes and which launches it makes, as pure host functions next to rf_configs.h
// (plain C++, no HIP: tests/select_test.cpp walks them on the CPU).  The launchers of rf_k_*.hip turn what these return into kernel
// instantiations (rf_tile_launch.h); the CPU emulator (emu/rf_emu.cpp) turns the same answers into loops over tiles.  Nothing else in
// the tree decides between two tiled kernels.
#pragma once
#include <type_traits>
#include "rf_configs.h"

namespace rf {

// ---- dtype and axis length: runtime value -> compile-time tag, each list expanded once -----------------------------------------
template <typename T> struct Real {
  using type = T;
  using cx = cplx<T>;
  static cx* p(void* v) { return static_cast<cx*>(v); }
  static const cx* p(const void* v) { return static_cast<const cx*>(v); }
  static cx* const* p(void* const* v) { return reinterpret_cast<cx* const*>(v); }
};
// f(Real<float>{}) or f(Real<double>{})
template <class F> auto with_real(int f64, F&& f) { return f64 ? f(Real<double>{}) : f(Real<float>{}); }

template <int N> using Size = std::integral_constant<int, N>;
// f(Size<+1>{}) (inverse) or f(Size<-1>{}) (forward)
template <class F> auto with_dir(int dir, F&& f) { return dir > 0 ? f(Size<+1>{}) : f(Size<-1>{}); }
// f(Size<N>{}) for a served length, `otherwise` for any other
#define RF_SIZE_CASE(NN) case NN: return f(Size<NN>{});
template <class R, class F> R for_col_size(int N, R otherwise, F&& f) {
  switch (N) { RF_COL_SIZES(RF_SIZE_CASE) default: return otherwise; }
}
template <class R, class F> R for_row_size(int M, R otherwise, F&& f) {
  switch (M) { RF_ROW_SIZES(RF_SIZE_CASE) default: return otherwise; }
}
template <class R, class F> R for_rowc_size(int M, R otherwise, F&& f) {
  switch (M) { RF_ROWC_SIZES(RF_SIZE_CASE) default: return otherwise; }
}
#undef RF_SIZE_CASE
template <class C> struct Cfg { using type = C; };
// f(Real<T>{}, Cfg<the row configuration>{}) for rows of M complex of either dtype
template <class R, class F> R for_rows(int f64, int M, R otherwise, F&& f) {
  return with_real(f64, [&](auto r) {
    return for_row_size(M, otherwise, [&](auto m) { return f(r, Cfg<typename RowSel<typename decltype(r)::type, decltype(m)::value>::type>{}); });
  });
}
// f(Real<T>{}, Cfg<SEL<T, N>::type>{}) for a strided pass of length N of either dtype (SEL: ColSel or GenSel)
template <template <typename, int> class SEL, class R, class F> R for_cols(int f64, int N, R otherwise, F&& f) {
  return with_real(f64, [&](auto r) {
    return for_col_size(N, otherwise, [&](auto n) { return f(r, Cfg<typename SEL<typename decltype(r)::type, decltype(n)::value>::type>{}); });
  });
}

// ---- shapes a pass can serve: pure arithmetic on the configurations --------------------------------------------------------------
// tile width (columns) of the strided pass of length N, and of the generation-fused x pass; 0 if unsupported
inline int col_tile_cols(int f64, int N) { return for_cols<ColSel>(f64, N, 0, [](auto, auto c) { return (int)decltype(c)::type::TC; }); }
inline int col_gen_tile_cols(int f64, int N) { return for_cols<GenSel>(f64, N, 0, [](auto, auto c) { return (int)decltype(c)::type::TC; }); }
// rows of x per block of the transposed intermediate (rf_fft.h xblock_x_geom): `want` if the last pass's uniform row offsets (multiples
// of N / RL) are whole blocks, else N (no blocking)
inline int col_gen_row_block(int f64, int N, int want) {
  if (want <= 0 || want >= N || (want & (want - 1))) return N;
  return for_cols<GenSel>(f64, N, N, [&](auto, auto c) { using C = typename decltype(c)::type; return (C::NPASS >= 2 && (C::N / C::RL) % want == 0) ? want : N; });
}
// can the strided pass of length N address this geometry?  (32-bit lane offsets everywhere; 64-bit ones exist for N >= 1024)
inline bool col_plain_addressable(int f64, int N, ColGeom g) {
  return for_cols<ColSel>(f64, N, false, [&](auto r, auto c) {
    using C = typename decltype(c)::type;
    return C::N >= 1024 || !g.needs_wide(C::LMAX, C::TC, (int)sizeof(typename decltype(r)::cx));
  });
}
// can the pass of length N store tile by tile to per-x-plane destinations?  (a tile must not straddle two x planes)
inline bool col_direct_supported(int f64, int N, long long inner) {
  const int tc = col_tile_cols(f64, N);
  return tc > 0 && inner > 0 && (inner & (inner - 1)) == 0 && inner % tc == 0;
}
// can the gathering z pass of rows of M complex serve tiles of tc columns and x blocks of rb rows?  (whole workgroups per (x block, iy))
inline bool row_c2r_xgather_ok(int f64, int M, int tc, int rb) {
  return for_rows(f64, M, false, [&](auto, auto c) { return tc > 0 && rb > 0 && rb % decltype(c)::type::NRT == 0 && M % tc == 0; });
}
// tiles (workgroups, moment partials) of the z pass over nrows rows; -1 if unsupported
inline long long row_c2r_tiles(int f64, int M, long long nrows) {
  return for_rows(f64, M, -1LL, [&](auto, auto c) { constexpr int NRT = decltype(c)::type::NRT; return (nrows + NRT - 1) / NRT; });
}
// the lognormal z pass: float64 rows of >= 512 complex keep the exp table in the tile's spare LDS slots (rf_fft.h LognormalRowIO)
template <typename T, int MM> using LognormalIO = LognormalRowIO<T, (sizeof(T) == 8 && MM >= 512) ? 1 : 0>;
// the shape part of "the x pass hands over through the blocked intermediate" (DESIGN.md section 3.8): x and y tiles of the same width,
// kz runs of whole tiles, and a z pass that can gather.  nzl: kz planes of the x / y passes, nzc = nz / 2: the z pass's rows
inline bool xpose_shape_ok(int f64, int nx, int ny, long long nzl, long long nzc, int row_block) {
  const int tcx = col_gen_tile_cols(f64, nx), tcy = col_tile_cols(f64, ny);
  return tcx > 0 && tcx == tcy && nzl >= tcx && nzl % tcx == 0 && row_c2r_xgather_ok(f64, (int)nzc, tcx, row_block);
}

// ---- the Col2 rule: which in-place (and direct) pass runs as two half-length transforms per tile ------------------------------
// float32 only: length 2048 on the radix-8-first 1024-point configuration (with 32 parked registers the 16-first one would not fit
// 128 VGPRs), length 1024 on PairSel1024.  launch_col_plain, launch_col_direct and the merged y+z launch all ask here, so the
// arithmetic per tile is the same in all three.
enum ColHalves { HALVES_NONE = 0, HALVES_OF_2048, HALVES_OF_1024 };
template <int H> struct HalvesSel;
template <> struct HalvesSel<HALVES_OF_2048> { using type = GenSel<float, 1024>::type; };
template <> struct HalvesSel<HALVES_OF_1024> { using type = PairSel1024::type; };
inline ColHalves col_halves(int f64, int N) {
  if (f64) return HALVES_NONE;
  if (RF_COL2_2048 && N == 2048) return HALVES_OF_2048;
  if (RF_Y_COL2_1024 && N == 1024) return HALVES_OF_1024;
  return HALVES_NONE;
}
// ... and can the halves of configuration C1 address this geometry?  (32-bit lane offsets for both the half's rows, two apart, and
// the whole column's; the plain column layout)  A geometry that does not fit keeps the whole-column kernel.
template <class C1> bool halves_fit(const ColGeom& g) {
  ColGeom gin = g;
  gin.row_stride = 2 * g.row_stride;
  const int eb = (int)sizeof(cplx<typename C1::T>);
  return !gin.needs_wide(C1::LMAX, C1::TC, eb) && !g.needs_wide(C1::LMAX, C1::TC, eb) && g.row_shift >= 30 && g.hi_shift >= 62 && g.sub_shift == 0;
}
// f(Cfg<half configuration>{}) for a length that has a halves form (any geometry), else nothing; was f called?
template <class F> bool for_col_halves(int f64, int N, F&& f) {
  switch (col_halves(f64, N)) {
    case HALVES_OF_2048: f(Cfg<HalvesSel<HALVES_OF_2048>::type>{}); return true;
    case HALVES_OF_1024: f(Cfg<HalvesSel<HALVES_OF_1024>::type>{}); return true;
    default: return false;
  }
}
// the same for a pass over geometry g: f is called when the length has a halves form AND g fits it
template <class F> bool for_col_halves(int f64, int N, const ColGeom& g, F&& f) {
  bool fit = false;
  for_col_halves(f64, N, [&](auto c) { if ((fit = halves_fit<typename decltype(c)::type>(g))) f(c); });
  return fit;
}

// ---- the y / z passes slab by slab: the partition of the nx planes ---------------------------------------------------------------
// planes: x planes per slab as asked for (<= 0 or >= nx: whole-grid passes); blocked: the x pass left its output in the blocked
// intermediate, whose slabs are whole x blocks of row_block rows, a power of two of them, dividing nx -- any other size: one slab.
// The last slab may be smaller.
struct YzSlabs { int planes, count, last; };      // planes per slab, number of slabs, planes of the last one
inline YzSlabs yz_slabs(int nx, long long planes, bool blocked, int row_block) {
  long long B = planes;
  if (blocked && B > 0 && (B % row_block || (B & (B - 1)) || nx % B)) B = 0;
  if (B <= 0 || B >= nx) B = nx;
  const int count = (int)((nx + B - 1) / B);
  return YzSlabs{(int)B, count, (int)(nx - (long long)(count - 1) * B)};
}

// ---- the fast generation pass: which kernel variant ------------------------------------------------------------------------------
// does the pass of this length fit a CU's LDS (tile + twiddles + the generation tables)?  false: float64, N = 2048 (and any N not served)
inline bool fastgen_supported(int f64, int N) {
  return with_real(f64, [&](auto r) {
    using T = typename decltype(r)::type;
    return for_col_size(N, false, [](auto n) { return GenSel<T, decltype(n)::value>::type::LDS_BYTES + FAST_LDS_BINS * (int)sizeof(FastRec) <= 160 * 1024; });
  });
}
inline bool col_fastgen_supported(int f64, int N) { return fastgen_supported(f64, N); }
// replicated-generation mode stores rows [rank N/P, (rank+1) N/P) only and tests the row offset m * L of the last pass: available when
// the x pass has an LDS stage and N/P is a multiple of L = N / (radix of the last pass)
inline bool col_replicate_supported(int f64, int N, int nranks) {
  if (!fastgen_supported(f64, N) || nranks < 1 || N % nranks) return false;
  return for_col_size(N, false, [&](auto n) { using C = typename GenSel<float, decltype(n)::value>::type; return C::NPASS >= 2 && (C::N / nranks) % (C::N / C::RL) == 0; });
}
// slab: the SLAB instantiations guard their stores (replicated generation); pot: 1 = the pass also stores delta(k) / k^2, 2 = it
// transforms pscale * delta(k) / k^2 instead; src: 0 native generator, 1 resident float64 deviates, 2 resident float32 pairs;
// halves: Col2 on the half-length configuration (float32: GenSel<float, 1024> for N = 2048; float64: GenSel<double, 512> for 1024)
struct FastVariant {
  bool valid;
  int slab, pot, src;
  bool halves;
};
inline bool operator==(const FastVariant& a, const FastVariant& b) {
  return a.valid == b.valid && (!a.valid || (a.slab == b.slab && a.pot == b.pot && a.src == b.src && a.halves == b.halves));
}
constexpr int fastgen_halves_length(int f64) { return f64 ? 1024 : 2048; }   // the length whose pass has a halves form (on GenSel of half of it)
// emit: the pass transforms the scaled potential (rf_realise_scaled_potential); noise64 / noise32: resident deviates are the source;
// pot: a potential array is stored next to the field; slab: only rows [x0, x1) are kept.  First match wins.
inline FastVariant fastgen_variant(int f64, int N, bool emit, bool noise64, bool noise32, bool pot, bool slab) {
  const FastVariant invalid{false, 0, 0, 0, false};
  auto whole = [](int s, int p, int src) { return FastVariant{true, s, p, src, false}; };
  auto halves = [](int p) { return FastVariant{true, 0, p, 0, true}; };
  if (!fastgen_supported(f64, N)) return invalid;                   // the caller keeps the exact kernel
  const bool two = N == fastgen_halves_length(f64) && (f64 || RF_COL2_2048);
  if (f64) {
    if (noise64 || noise32) return invalid;                         // resident deviates: the exact kernel serves float64 plans
    if (emit) return (slab || pot) ? invalid : two ? halves(2) : whole(0, 2, 0);
    if (pot) return slab ? invalid : whole(0, 1, 0);                // the second store stream: the whole-column kernel
    if (two && !slab) return halves(0);
    return slab ? whole(1, 0, 0) : whole(0, 0, 0);
  }
  if (emit) {
    if (slab || pot || noise64) return invalid;
    return noise32 ? whole(0, 2, 2) : two ? halves(2) : whole(0, 2, 0);
  }
  if (noise64) return (slab || pot) ? invalid : whole(0, 0, 1);     // rng='reference' through the fast float32 sigma path
  if (noise32) return slab ? invalid : whole(0, pot ? 1 : 0, 2);
  if (pot) return slab ? invalid : whole(0, 1, 0);                  // generation + potential store (save_potential=True), whole grid
  if (slab) return whole(1, 0, 0);
  return two ? halves(0) : whole(0, 0, 0);
}
// The variants that exist as kernels, one compile-time list per dtype: the launch path picks its entry by value, plan creation walks
// the whole list (the halves entries count for N = fastgen_halves_length only).
template <int SLAB, int POT, int SRC, bool HALVES> struct FastV {
  static constexpr int slab = SLAB, pot = POT, src = SRC;
  static constexpr bool halves = HALVES;
  static constexpr FastVariant value() { return FastVariant{true, SLAB, POT, SRC, HALVES}; }
};
template <class... V> struct FastList {};
using FastList32 = FastList<FastV<0, 2, 2, false>, FastV<0, 2, 0, false>, FastV<0, 0, 1, false>, FastV<0, 0, 2, false>, FastV<0, 1, 2, false>,
                            FastV<0, 1, 0, false>, FastV<1, 0, 0, false>, FastV<0, 0, 0, false>, FastV<0, 2, 0, true>, FastV<0, 0, 0, true>>;
using FastList64 = FastList<FastV<0, 2, 0, false>, FastV<0, 1, 0, false>, FastV<1, 0, 0, false>, FastV<0, 0, 0, false>, FastV<0, 2, 0, true>,
                            FastV<0, 0, 0, true>>;
template <typename T> using FastListOf = std::conditional_t<sizeof(T) == 8, FastList64, FastList32>;
// f(V{}) for the entry equal to v; `otherwise` when v is invalid or not in the list
template <class R, class F, class... V> R with_fast_variant(FastList<V...>, const FastVariant& v, R otherwise, F&& f) {
  R r = otherwise;
  (void)(... || (v.valid && V::value() == v && ((r = f(V{})), true)));
  return r;
}
// f(V{}) for every entry while it returns `ok`; the first other result, else `ok`
template <class R, class F, class... V> R for_each_fast_variant(FastList<V...>, R ok, F&& f) {
  R r = ok;
  (void)(... && ((r = f(V{})) == ok));
  return r;
}

// ---- the fast generation pass: its one to three launches ------------------------------------------------------------------------
// The tiles that hold slot kz = 0 (one per ky row when a tile is narrower than a kz row) run FIRST, as a launch of their own by the
// kernel with the Hermitian repair; every other tile by the lean kernel without it (skip_period = tiles per ky row).  The long passes'
// repair kernel takes the repaired slots from a side buffer that a fill kernel writes in front of it.
enum FastKind { FAST_FIX_FILL, FAST_COL, FAST_COLPAIR, FAST_COL2 };
enum FastIo { FAST_IO_LEAN, FAST_IO_REPAIR, FAST_IO_FIRST };   // FIX = 0; FIX = 1; the kz = 0 launch's own: FIX = 3 (side buffer) or 1
struct FastStep {
  int kind, io;
  long long count, mul, add;      // tiles (pairs) b * mul + add, b in [0, count)
  int skip_period;                // > 0: every tile (pair) except those = 0 mod skip_period
  bool record_after;              // the caller's `after_repair` event goes here
};
struct FastSequence {
  bool valid;
  int n;
  FastStep step[3];
};
// what the configuration contributes: tile columns; side = the kz = 0 launch reads the side buffer (long passes), else its owning lane
// repairs; pairs = a tile-pair kernel exists; halves = Col2
struct FastPass { int tc; bool side, pairs, halves; };
// ... of configuration C (halves: C is the half-length configuration) with deviate source src.  The long passes read the side buffer;
// the short ones (a few tiles, one pass) keep the owning lane's repair.  Tile pairs with whole-line stores (rf_fft.h ColPair): the
// 1024-point float32 whole-column pass on the native generator or float32 deviates.
template <class C> constexpr FastPass fast_pass_of(bool halves, int src) {
  constexpr bool side = C::N >= 512 && C::NPASS >= 2;
  return FastPass{C::TC, side, !halves && side && C::N == 1024 && sizeof(typename C::T) == 4 && C::NPASS == 3 && (src == 0 || src == 2), halves};
}
// full_rows: every x row is kept (no replicated-generation slab)
inline FastSequence fastgen_sequence(const FastPass& c, int nzl, long long ncols, int kz0, bool full_rows, const ColGeom& g, bool have_fixbuf) {
  FastSequence q{true, 0, {}};
  const FastSequence invalid{false, 0, {}};
  const int one = c.halves ? FAST_COL2 : FAST_COL;
  auto add = [&](int kind, int io, long long count, long long mul, int skip, bool rec) { q.step[q.n++] = FastStep{kind, io, count, mul, 0, skip, rec}; };
  const bool split = nzl > c.tc && nzl % c.tc == 0;
  const long long tiles_per_iy = nzl / c.tc, ntiles = ncols / c.tc;
  if (!split) { add(one, FAST_IO_REPAIR, ntiles, 1, 0, false); return q; }
  // tile pairs with whole-line stores: every tile of a kz row in a pair of its own row
  const bool use_pairs = c.pairs && full_rows && tiles_per_iy % 2 == 0 && g.inner % (2 * c.tc) == 0 && g.sub_shift == 0;
  if (kz0 != 0) {                                                       // only the slab that owns kz = 0 needs the repair
    if (use_pairs && ntiles / 2 < (1LL << 31)) add(FAST_COLPAIR, FAST_IO_LEAN, ntiles / 2, 1, 0, false);
    else add(one, FAST_IO_LEAN, ntiles, 1, 0, false);
    return q;
  }
  if (c.side) {
    if (!have_fixbuf) return invalid;
    add(FAST_FIX_FILL, FAST_IO_REPAIR, 0, 1, 0, false);
  }
  if (use_pairs) {
    // the pair that holds the kz = 0 tile of every ky row (only that tile's owning lanes take the repair), then all others
    const long long ppi = tiles_per_iy / 2, npairs = ntiles / 2;
    if (ppi >= (1LL << 30) || npairs >= (1LL << 31)) return invalid;
    add(FAST_COLPAIR, FAST_IO_FIRST, ncols / nzl, ppi, 0, true);
    if (ppi >= 2) add(FAST_COLPAIR, FAST_IO_LEAN, npairs - npairs / ppi, 1, (int)ppi, false);   // (ppi = 1: the first launch has covered everything)
    return q;
  }
  if (tiles_per_iy >= (1LL << 30) || ntiles >= (1LL << 31)) return invalid;
  add(one, FAST_IO_FIRST, ncols / nzl, tiles_per_iy, 0, true);
  add(one, FAST_IO_LEAN, ntiles - ntiles / tiles_per_iy, 1, (int)tiles_per_iy, false);
  return q;
}
// the tile (pair) that workgroup-order index b of a step runs, as the kernels compute it (rf_kernels.h col_kernel) without the XCD deal
inline long long fast_step_tile(const FastStep& s, long long b) {
  long long t = b * s.mul + s.add;
  if (s.skip_period > 0) t = t + t / (s.skip_period - 1) + 1;
  return t;
}

// ---- the fast generation pass: the types of one variant at one length -------------------------------------------------------------
template <class IO, class = void> struct io_noise_src { static constexpr int value = 0; };
template <class IO> struct io_noise_src<IO, typename std::enable_if<(IO::NOISE_SRC >= 0)>::type> { static constexpr int value = IO::NOISE_SRC; };
// One variant on configuration C (HALVES: C is the half-length configuration of a Col2 pass).  IOT<FIX>: the variant's IO with that
// repair mode -- 0 none (lean), 1 the owning lane's own, 3 from the side buffer.
template <class C_, template <int> class IOT, bool HALVES_>
struct FastPassOf {
  using C = C_;
  using T = typename C::T;
  static constexpr bool HALVES = HALVES_;
  using IO0 = IOT<0>;
  using IO1 = IOT<1>;
  static constexpr FastPass pass = fast_pass_of<C>(HALVES, io_noise_src<IO0>::value);
  static constexpr bool side = pass.side, pairs = pass.pairs;
  // the kz = 0 launch: the repaired slots from the side buffer (FIX = 3, filled by fix_fill_kernel just before) or the owning lane's own
  using IOC = typename IO1::template with_fix<side ? 3 : 1>;
  using IOF = typename IO1::fill_io;
  // full_rows: every x row is kept.  The slab-restricted instantiations test the workgroup-uniform row offset m * L of the last pass: the
  // slab boundaries must be multiples of L = N / (radix of the last pass)
  static bool full_rows(int x0, int x1) { return x0 <= 0 && x1 >= (HALVES ? 2 : 1) * C::N; }
  static bool accepts(const ColGeom& g, long long ncols, int nzl, int x0, int x1) {
    if (nzl <= 0 || (nzl & (nzl - 1)) || ncols >= (1LL << 31) || g.needs_wide(C::LMAX, C::TC, (int)sizeof(cplx<T>))) return false;   // the IO splits a column index by shift and mask
    if (HALVES && !g.rows_ok(C::N / C::RL, C::NPASS)) return false;
    return full_rows(x0, x1) || !(HALVES || C::NPASS < 2 || x0 % (C::N / C::RL) || x1 % (C::N / C::RL));
  }
};
// the IO type of list entry V (FastListOf<T>) with repair mode FIX
template <typename T, class V, int FIX> struct FastIoOf { using type = FastGenColIOT<FIX, V::slab, V::pot, V::src, V::halves ? 2 : 1>; };
template <class V, int FIX> struct FastIoOf<double, V, FIX> { using type = FastGenColIO64<FIX, V::slab, V::pot, V::halves ? 2 : 1>; };
// One dtype's fast generation pass.  The halves form is Col2 on the configuration of half of NH (float64: length 1024 as two 512-point
// transforms per tile, two workgroups per CU -- DESIGN.md 3.10).
template <typename T> struct FastGen {
  static constexpr int NH = fastgen_halves_length(sizeof(T) == 8);
  using CHalf = typename GenSel<T, NH / 2>::type;
  template <class V> struct Bind { template <int FIX> using IO = typename FastIoOf<T, V, FIX>::type; };
  // f(Cfg<the FastPassOf of entry V at length N>{}); `otherwise` where V has no kernel at N
  template <class V, class R, class F> static R at(int N, R otherwise, F&& f) {
    if constexpr (V::halves) return N == NH ? f(Cfg<FastPassOf<CHalf, Bind<V>::template IO, true>>{}) : otherwise;
    else return for_col_size(N, otherwise, [&](auto n) { return f(Cfg<FastPassOf<typename GenSel<T, decltype(n)::value>::type, Bind<V>::template IO, false>>{}); });
  }
};

}  // namespace rf
