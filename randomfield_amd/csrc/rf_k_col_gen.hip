// x pass of the c2r transform with generation (rows K,T,R,S) fused into its load: float32 kernels and the exact-chain kernels
// (the float64 fast-generation kernels live in rf_k_col_gen64.hip: see rf_col_gen_launch.h)
#include "rf_col_gen_launch.h"

namespace rf {
namespace {
template <class V, int FIX> struct FastIo32 { using type = FastGenColIOT<FIX, V::slab, V::pot, V::src, V::halves ? 2 : 1>; };
using Fast32 = FastGen<float, FastIo32>;

template <typename T, bool WIDE> GenColIO<T, WIDE> gen_io(cplx<T>* W, ColGeom g, const GenParams& gp, const cplx<T>* kspace, int kz0, int nzl) {
  GenColIO<T, WIDE> io; io.base = W; io.g = g; io.gp = gp; io.kspace = kspace; io.kz0 = kz0; io.nzl = nzl;
  return io;
}
// the exact pass has 64-bit lane offsets where a packed plan can need them: float64, length 2048
template <typename T, int NN> constexpr bool gen_has_wide = NN == 2048 && sizeof(T) == 8;
}  // namespace

// x pass fused with the fast native generation: the variant by rf_select.h fastgen_variant, float32 here and float64 in rf_k_col_gen64.hip
hipError_t launch_col_fastgen(int f64, int N, void* W, ColGeom g, long long ncols, const FastGenParams& gp, int kz0, int nzl,
                              const void* tw, hipStream_t s, hipEvent_t after_repair, int x0, int x1, void* pot, void* fixbuf) {
  const bool slab = x0 > 0 || x1 < N;          // replicated-generation mode
  const FastVariant v = fastgen_variant(f64, N, gp.emit_potential != 0, gp.noise != nullptr, gp.noise32 != nullptr, pot != nullptr, slab);
  if (!v.valid) return hipErrorInvalidValue;
  if (f64) return launch_col_fastgen64(N, v, W, g, ncols, gp, kz0, nzl, tw, s, after_repair, x0, x1, pot, fixbuf);
  using R = Real<float>;
  return Fast32::launch(N, v, FastArgs<float>{gp, R::p(W), g, ncols, kz0, nzl, R::p(tw), s, after_repair, x0, x1, R::p(pot), R::p(fixbuf)});
}

int col_gen_tile_cols(int f64, int N) {
  return with_real(f64, [&](auto r) {
    return for_col_size(N, 0, [&](auto n) { return (int)GenSel<typename decltype(r)::type, decltype(n)::value>::type::TC; });
  });
}

// rows of x per block of the transposed intermediate (rf_fft.h xpose_store_geom): `want` if the last pass's uniform row
// offsets (multiples of N / RL) are whole blocks, else N (no blocking)
int col_gen_row_block(int f64, int N, int want) {
  if (want <= 0 || want >= N || (want & (want - 1))) return N;
  return with_real(f64, [&](auto r) {
    return for_col_size(N, N, [&](auto n) {
      using C = typename GenSel<typename decltype(r)::type, decltype(n)::value>::type;
      return (C::NPASS >= 2 && (C::N / C::RL) % want == 0) ? want : N;
    });
  });
}

// does the fast-generation x pass of this length fit a CU's LDS (tile + twiddles + the generation tables)?
bool col_fastgen_supported(int f64, int N) { return fastgen_supported(f64, N); }

// replicated-generation mode stores rows [rank N/P, (rank+1) N/P) only and tests the row offset m * L of the last pass:
// available when the x pass has an LDS stage and N/P is a multiple of L = N / (radix of the last pass)
bool col_replicate_supported(int f64, int N, int nranks) {
  if (!col_fastgen_supported(f64, N) || nranks < 1 || N % nranks) return false;
  return for_col_size(N, false, [&](auto n) { using C = typename GenSel<float, decltype(n)::value>::type; return C::NPASS >= 2 && (C::N / nranks) % (C::N / C::RL) == 0; });
}

// x pass of c2r fused with generation (kspace == nullptr) or reading an API-layout k array: the exact dtype chain
hipError_t launch_col_gen(int f64, int N, void* W, ColGeom g, long long ncols, const GenParams& gp,
                          const void* kspace, int kz0, int nzl, const void* tw, hipStream_t s) {
  return with_real(f64, [&](auto r) {
    using R = decltype(r); using T = typename R::type;
    return for_col_size(N, hipErrorInvalidValue, [&](auto n) {
      constexpr int NN = decltype(n)::value;
      using C = typename GenSel<T, NN>::type;
      if (g.needs_wide(C::LMAX, C::TC, (int)sizeof(cplx<T>))) {
        if constexpr (gen_has_wide<T, NN>) return launch_col<C>(gen_io<T, true>(R::p(W), g, gp, R::p(kspace), kz0, nzl), ncols, R::p(tw), s, ncols / C::TC);
        return hipErrorInvalidValue;
      }
      return launch_col<C>(gen_io<T, false>(R::p(W), g, gp, R::p(kspace), kz0, nzl), ncols, R::p(tw), s, ncols / C::TC);
    });
  });
}

hipError_t prepare_col_gen(int f64, int N) {
  Prepare p;
  with_real(f64, [&](auto r) {
    using T = typename decltype(r)::type;
    return for_col_size(N, 0, [&](auto n) {
      constexpr int NN = decltype(n)::value;
      using C = typename GenSel<T, NN>::type;
      if constexpr (gen_has_wide<T, NN>) p.kernel<col_kernel<C, +1, GenColIO<T, true>>>(lds_of<C, GenColIO<T, true>>());
      p.kernel<col_kernel<C, +1, GenColIO<T>>>(lds_of<C, GenColIO<T>>());
      return 0;
    });
  });
  if (p.e != hipSuccess || !fastgen_supported(f64, N)) return p.e;
  return f64 ? prepare_col_fastgen64(N) : Fast32::prepare(N);
}
}  // namespace rf
