// x pass of the c2r transform with generation (rows K,T,R,S) fused into its load: float32 kernels and the exact-chain kernels
// (the float64 fast-generation kernels live in rf_k_col_gen64.hip: see rf_col_gen_launch.h)
#include "rf_col_gen_launch.h"

namespace rf {
namespace {
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
  return fastgen_launch<float>(N, v, FastArgs<float>{{gp, R::p(W), g, kz0, nzl, x0, x1, R::p(pot), R::p(fixbuf)}, ncols, R::p(tw), s, after_repair});
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
        if constexpr (gen_has_wide<T, NN>) return launch_col<C>(gen_col_io<T, true>(R::p(W), g, gp, R::p(kspace), kz0, nzl), ncols, R::p(tw), s, ncols / C::TC);
        return hipErrorInvalidValue;
      }
      return launch_col<C>(gen_col_io<T, false>(R::p(W), g, gp, R::p(kspace), kz0, nzl), ncols, R::p(tw), s, ncols / C::TC);
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
  return f64 ? prepare_col_fastgen64(N) : fastgen_prepare<float>(N);
}
}  // namespace rf
