// strided in-place FFT passes (PlainColIO), float32 + float64, both directions
#include "rf_tile_launch.h"

namespace rf {
namespace {
template <class C, int DIR, class IO>
hipError_t launch_one(const IO& io, long long ncols, const cplx<typename C::T>* tw, hipStream_t s) {
  if (ncols % C::TC || !pow2(io.g.inner)) return hipErrorInvalidValue;
  const long long ntiles = ncols / C::TC;
  return tile_launch<col_kernel<C, DIR, IO>>(ntiles, C::NT, lds_of<C, IO>(), s, io, tw, ntiles, 1LL, 0LL, 0);
}
// the in-place pass on whole columns: 64-bit lane offsets exist for N >= 1024 (the long axes of the largest arrays: unpacked c2c, float64)
template <typename T, int DIR>
hipError_t launch_whole(int N, cplx<T>* base, ColGeom g, long long ncols, const cplx<T>* tw, hipStream_t s) {
  return for_col_size(N, hipErrorInvalidValue, [&](auto n) {
    constexpr int NN = decltype(n)::value;
    using C = typename ColSel<T, NN>::type;
    if (g.needs_wide(C::LMAX, C::TC, (int)sizeof(cplx<T>))) {
      if constexpr (NN >= 1024) {
        PlainColIO<T, true> iow; iow.base = base; iow.g = g;
        return launch_one<C, DIR>(iow, ncols, tw, s);
      }
      return hipErrorInvalidValue;
    }
    PlainColIO<T> io; io.base = base; io.g = g;
    return launch_one<C, DIR>(io, ncols, tw, s);
  });
}
// a pass of length 2 C1::N in place as two C1 transforms per tile (rf_fft.h Col2 / Pair2ColIO); tw2 = the 2 C1::N-point table
template <class C1, int DIR>
hipError_t launch_pair(cplx<float>* base, ColGeom g, long long ncols, const cplx<float>* tw2, hipStream_t s) {
  using IO = Pair2ColIO<float>;
  if (ncols % C1::TC || !pow2(g.inner)) return hipErrorInvalidValue;
  const long long ntiles = ncols / C1::TC;
  return tile_launch<col2_kernel<C1, DIR, IO>>(ntiles, C1::NT, lds_of<C1, IO>(), s, pair2_col_io<IO>(base, g), tw2, ntiles, 1LL, 0LL, 0);
}
}  // namespace

// inverse pass in place + the Parseval partials (AccColIO)
hipError_t launch_col_plain_acc(int f64, int N, void* base, ColGeom g, long long ncols, int kz0, int nzl, double* partials, const void* tw,
                                hipStream_t s) {
  if (!pow2(nzl)) return hipErrorInvalidValue;
  return with_real(f64, [&](auto r) {
    using R = decltype(r); using T = typename R::type;
    const AccColIO<T> io = acc_col_io(R::p(base), g, partials, kz0, nzl);
    return for_col_size(N, hipErrorInvalidValue, [&](auto n) {
      using C = typename ColSel<T, decltype(n)::value>::type;
      if (g.needs_wide(C::LMAX, C::TC, (int)sizeof(cplx<T>))) return hipErrorInvalidValue;
      return launch_one<C, +1>(io, ncols, R::p(tw), s);
    });
  });
}

// inverse pass out of place: src (geometry gs) -> dst (geometry gd)
hipError_t launch_col_xpose(int f64, int N, const void* src, ColGeom gs, void* dst, ColGeom gd, long long ncols, const void* tw,
                            hipStream_t s) {
  if (gd.inner <= 0 || ncols % gd.inner) return hipErrorInvalidValue;
  const long long nhi = ncols / gd.inner;                 // values of the slow index (ix); gd.inner = kz planes per run
  if (nhi & (nhi - 1)) return hipErrorInvalidValue;
  return with_real(f64, [&](auto r) {
    using R = decltype(r); using T = typename R::type;
    return for_col_size(N, hipErrorInvalidValue, [&](auto n) {
      using C = typename ColSel<T, decltype(n)::value>::type;
      if (gs.needs_wide(C::LMAX, C::TC, (int)sizeof(cplx<T>)) || gd.needs_wide(C::LMAX, C::TC, (int)sizeof(cplx<T>)) || !pow2(gs.inner) ||
          (gs.sub_shift > 0 && (1 << gs.sub_shift) < C::TC) || gd.inner % C::TC)
        return hipErrorInvalidValue;
      return launch_one<C, +1>(xpose_col_io(R::p(src), gs, R::p(dst), gd, ncols, C::TC), ncols, R::p(tw), s);
    });
  });
}

// RF_Y_COL2_1024 (rf_configs.h): the float32 in-place pass of length 1024 as two 512-point transforms per 8-column tile (Col2): 256
// threads, 36 KB of LDS, 109 registers -- FOUR workgroups per CU where the whole-column kernel (72 KB) has two.  The pass is
// latency-bound, not HBM-bound (its slab is read once from HBM and handed to the z pass through the Infinity Cache): more tiles in
// flight per CU, y pass 1.70 -> 1.61 ms per 1024^3 (profiles/r04_ab/ycol2.log).  Which lengths and geometries: rf_select.h col_halves.
hipError_t launch_col_plain(int f64, int N, int dir, void* base, ColGeom g, long long ncols, const void* tw, hipStream_t s) {
  return with_dir(dir, [&](auto d) {
    constexpr int DIR = decltype(d)::value;
    hipError_t e = hipSuccess;
    if (for_col_halves(f64, N, g, [&](auto c) { e = launch_pair<typename decltype(c)::type, DIR>((cplx<float>*)base, g, ncols, (const cplx<float>*)tw, s); }))
      return e;
    return with_real(f64, [&](auto r) { using R = decltype(r); return launch_whole<typename R::type, DIR>(N, R::p(base), g, ncols, R::p(tw), s); });
  });
}

// every kernel the in-place pass of (dtype, N, dir) can launch; with `inverse_forms` the out-of-place and the accumulating pass too
hipError_t prepare_col_plain(int f64, int N, int dir, bool inverse_forms) {
  Prepare p;
  with_dir(dir, [&](auto d) {
    constexpr int DIR = decltype(d)::value;
    for_col_halves(f64, N, [&](auto c) { using C1 = typename decltype(c)::type; p.kernel<col2_kernel<C1, DIR, Pair2ColIO<float>>>(lds_of<C1, Pair2ColIO<float>>()); });
    with_real(f64, [&](auto r) {
      using T = typename decltype(r)::type;
      return for_col_size(N, 0, [&](auto n) {
        constexpr int NN = decltype(n)::value;
        using C = typename ColSel<T, NN>::type;
        if constexpr (NN >= 1024) p.kernel<col_kernel<C, DIR, PlainColIO<T, true>>>(lds_of<C, PlainColIO<T, true>>());
        p.kernel<col_kernel<C, DIR, PlainColIO<T>>>(lds_of<C, PlainColIO<T>>());
        if constexpr (DIR > 0) {
          if (inverse_forms) {
            p.kernel<col_kernel<C, +1, XposeColIO<T>>>(lds_of<C, XposeColIO<T>>());
            p.kernel<col_kernel<C, +1, AccColIO<T>>>(lds_of<C, AccColIO<T>>());
          }
        }
        return 0;
      });
    });
    return 0;
  });
  return p.e;
}
}  // namespace rf
