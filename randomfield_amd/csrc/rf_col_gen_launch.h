// rf_col_gen_launch.h -- launch helpers shared by the two translation units of the generation pass (rf_k_col_gen.hip: float32,
// compiled with the max-ILP scheduling strategy; rf_k_col_gen64.hip: float64, default strategy -- measured on MI355X: the float32
// whole-column kernels gain 7 % from it, the float64 half-transform kernels lose 8 %)
#pragma once
#include "rf_tile_launch.h"

// (Launch structure of the kz = 0 repair, settled by measurement -- DESIGN_HISTORY.md: the tiles that hold slot kz = 0 run as a launch of
// their own in FRONT of the lean kernel's launch over all other tiles.  One launch of the repairing kernel over all tiles, the lean
// kernel over all tiles followed by the kz = 0 tiles again, and both kinds of tile in one grid were each measured and are gone.)
// Which variant: rf_select.h fastgen_variant; which launches: fastgen_sequence.  This file turns both into kernels.

namespace rf {
namespace {
// runs tiles  b * tile_mul + tile_add,  b in [0, ntiles)
template <class C, class IO>
hipError_t launch_col(const IO& io, long long ncols, const cplx<typename C::T>* tw, hipStream_t s, long long ntiles, long long tile_mul = 1,
                      long long tile_add = 0, int skip_period = 0) {
  if (ncols % C::TC || !pow2(io.g.inner)) return hipErrorInvalidValue;
  if (!io.g.rows_ok(C::N / C::RL, C::NPASS) || (io.g.sub_shift > 0 && (1 << io.g.sub_shift) < C::TC)) return hipErrorInvalidValue;
  return tile_launch<col_kernel<C, +1, IO>>(ntiles, C::NT, lds_of<C, IO>(), s, io, tw, ntiles, tile_mul, tile_add, skip_period);
}
// pairs of adjacent tiles, whole-line stores (rf_kernels.h colpair_kernel): runs pairs b * pair_mul + pair_add, b in [0, npairs)
// (the float32 generation pass of length 1024 -- native generator or replayed deviates, whole grid or kz slab -- runs on tile pairs)
template <class C, class IO>
hipError_t launch_colpair(const IO& io, long long ncols, const cplx<typename C::T>* tw, hipStream_t s, long long npairs, long long pair_mul,
                          long long pair_add, int skip_period) {
  if (ncols % (2 * C::TC) || !pow2(io.g.inner)) return hipErrorInvalidValue;
  if (!io.g.rows_ok(C::N / C::RL, C::NPASS) || io.g.sub_shift > 0 || io.g.inner % (2 * C::TC)) return hipErrorInvalidValue;
  return tile_launch<colpair_kernel<C, +1, IO>>(npairs, C::NT, lds_of<C, IO>(), s, io, tw, npairs, pair_mul, pair_add, skip_period);
}
// the same through col2_kernel: a pass of length 2 C1::N as two C1 transforms per tile (rf_fft.h Col2); tw2 = the 2 C1::N-point table
template <class C1, class IO>
hipError_t launch_col2(const IO& io, long long ncols, const cplx<typename C1::T>* tw2, hipStream_t s, long long ntiles, long long tile_mul,
                       long long tile_add, int skip_period) {
  if (ncols % C1::TC || !pow2(io.g.inner)) return hipErrorInvalidValue;
  return tile_launch<col2_kernel<C1, +1, IO>>(ntiles, C1::NT, lds_of<C1, IO>(), s, io, tw2, ntiles, tile_mul, tile_add, skip_period);
}

// what a fast generation pass is called with: the IO's contents (rf_fft_gen.h FastIoArgs) + the launch's own
template <typename T> struct FastArgs : FastIoArgs<T> {
  long long ncols;
  const cplx<T>* tw;
  hipStream_t s;
  hipEvent_t after_repair;
};

// The launches of one variant at one length: P = its rf_select.h FastPassOf (configuration, IO types, FastPass).
template <class P>
struct FastLaunch {
  using C = typename P::C;
  using T = typename P::T;
  using IO0 = typename P::IO0;
  using IO1 = typename P::IO1;
  using IOC = typename P::IOC;
  using IOF = typename P::IOF;
  static constexpr bool HALVES = P::HALVES;

  template <class IO> static hipError_t one(const FastArgs<T>& a, const FastStep& st) {
    if constexpr (HALVES) return launch_col2<C>(fast_col_io<IO>(a), a.ncols, a.tw, a.s, st.count, st.mul, st.add, st.skip_period);
    else return launch_col<C>(fast_col_io<IO>(a), a.ncols, a.tw, a.s, st.count, st.mul, st.add, st.skip_period);
  }
  static hipError_t step(const FastArgs<T>& a, const FastStep& st) {
    switch (st.kind) {
      case FAST_FIX_FILL:     // one thread per mode (rf_kernels.h fix_fill_kernel): out[iy * nx + ix]
        if constexpr (P::side) {
          const long long n = (long long)a.gp.nx * a.gp.ny;
          return tile_launch<fix_fill_kernel<IOF, cplx<T>>>((n + 255) / 256, 256, IOF::LDS_EXTRA, a.s, fast_col_io<IOF>(a), a.fixbuf, a.gp.nx, a.gp.ny);
        }
        return hipErrorInvalidValue;
      case FAST_COLPAIR:
        if constexpr (P::pairs) {
          if (st.io == FAST_IO_LEAN) return launch_colpair<C>(fast_col_io<IO0>(a), a.ncols, a.tw, a.s, st.count, st.mul, st.add, st.skip_period);
          if (st.io == FAST_IO_FIRST) return launch_colpair<C>(fast_col_io<IOC>(a), a.ncols, a.tw, a.s, st.count, st.mul, st.add, st.skip_period);
        }
        return hipErrorInvalidValue;
      default:
        return st.io == FAST_IO_LEAN ? one<IO0>(a, st) : st.io == FAST_IO_REPAIR ? one<IO1>(a, st) : one<IOC>(a, st);
    }
  }
  static hipError_t launch(const FastArgs<T>& a) {
    if (!P::accepts(a.g, a.ncols, a.nzl, a.x0, a.x1)) return hipErrorInvalidValue;
    const FastSequence q = fastgen_sequence(P::pass, a.nzl, a.ncols, a.kz0, P::full_rows(a.x0, a.x1), a.g, a.fixbuf != nullptr);
    if (!q.valid) return hipErrorInvalidValue;
    for (int i = 0; i < q.n; ++i) {
      if (hipError_t e = step(a, q.step[i]); e != hipSuccess) return e;
      if (q.step[i].record_after && a.after_repair)
        if (hipError_t e = hipEventRecord(a.after_repair, a.s); e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  static void prepare(Prepare& p) {
    if constexpr (HALVES) {
      p.kernel<col2_kernel<C, +1, IO0>>(lds_of<C, IO0>());
      p.kernel<col2_kernel<C, +1, IOC>>(lds_of<C, IOC>());
      p.kernel<col2_kernel<C, +1, IO1>>(lds_of<C, IO1>());
    } else {
      p.kernel<col_kernel<C, +1, IO0>>(lds_of<C, IO0>());
      if constexpr (P::pairs) {
        p.kernel<colpair_kernel<C, +1, IO0>>(lds_of<C, IO0>());
        p.kernel<colpair_kernel<C, +1, IOC>>(lds_of<C, IOC>());
      }
      p.kernel<col_kernel<C, +1, IOC>>(lds_of<C, IOC>());
      p.kernel<col_kernel<C, +1, IO1>>(lds_of<C, IO1>());
    }
  }
};

// One dtype's fast generation pass (rf_select.h FastGen<T>, FastListOf<T>): `launch` indexes the list by the variant chosen, `prepare` walks it.
template <typename T> hipError_t fastgen_launch(int N, const FastVariant& v, const FastArgs<T>& a) {
  return with_fast_variant(FastListOf<T>{}, v, hipErrorInvalidValue, [&](auto e) {
    return FastGen<T>::template at<decltype(e)>(N, hipErrorInvalidValue, [&](auto k) { return FastLaunch<typename decltype(k)::type>::launch(a); });
  });
}
template <typename T> hipError_t fastgen_prepare(int N) {
  Prepare p;
  for_each_fast_variant(FastListOf<T>{}, 0, [&](auto e) {
    return FastGen<T>::template at<decltype(e)>(N, 0, [&](auto k) { FastLaunch<typename decltype(k)::type>::prepare(p); return 0; });
  });
  return p.e;
}

}  // namespace

// the float64 half of launch_col_fastgen (rf_k_col_gen64.hip)
hipError_t launch_col_fastgen64(int N, const FastVariant& v, void* W, ColGeom g, long long ncols, const FastGenParams& gp, int kz0, int nzl, const void* tw,
                                hipStream_t s, hipEvent_t after_repair, int x0, int x1, void* pot, void* fixbuf);
}  // namespace rf
