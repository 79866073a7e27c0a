// z pass of the c2r transform (contiguous rows, Hermitian untangle fused, moments) and the forward z pass
#include "rf_tile_launch.h"

namespace rf {
namespace {
template <class C>
constexpr int row_lds_bytes() { return C::LDS_BYTES > 2 * (C::NT / 64) * 8 ? C::LDS_BYTES : 2 * (C::NT / 64) * 8; }
template <class C>
constexpr int fwd_lds_bytes() { return C::LDS_BYTES > 64 ? C::LDS_BYTES : 64; }
template <class C> long long row_tiles(long long nrows) { return (nrows + C::NRT - 1) / C::NRT; }

template <class C, class IO>
hipError_t launch_one(const IO& io, long long nrows, const cplx<typename C::T>* tw, double* partials, hipStream_t s) {
  return tile_launch<row_c2r_kernel<C, IO>>(row_tiles<C>(nrows), C::NT, row_lds_bytes<C>(), s, io, tw, nrows, partials);
}
}  // namespace

hipError_t launch_row_c2r(int f64, int M, void* W, long long nrows, double scale, const void* tw, double* partials, hipStream_t s) {
  return for_rows(f64, M, hipErrorInvalidValue, [&](auto r, auto c) {
    using R = decltype(r); using T = typename R::type;
    PlainRowIO<T> io; io.base = R::p(W); io.scale = (T)scale; io.M_of = M;
    return launch_one<typename decltype(c)::type>(io, nrows, R::p(tw), partials, s);
  });
}
hipError_t launch_row_c2r_gather(int f64, int M, const void* src, void* dst, long long nrows, double scale, int nzl,
                                 long long seg_stride, const void* tw, double* partials, hipStream_t s) {
  if (!pow2(nzl)) return hipErrorInvalidValue;       // (the kernel splits k by shift and mask)
  return for_rows(f64, M, hipErrorInvalidValue, [&](auto r, auto c) {
    using R = decltype(r); using T = typename R::type;
    return launch_one<typename decltype(c)::type>(gather_row_io(R::p(src), R::p(dst), scale, M, nzl, seg_stride), nrows, R::p(tw), partials, s);
  });
}
hipError_t launch_row_c2r_xgather(int f64, int M, const void* src, void* dst, long long nrows, double scale, int tc, int rb, int ny,
                                  const void* tw, double* partials, hipStream_t s) {
  if (!pow2(tc) || !pow2(rb) || !pow2(ny) || M % tc || nrows % rb) return hipErrorInvalidValue;
  return for_rows(f64, M, hipErrorInvalidValue, [&](auto r, auto c) {
    using R = decltype(r); using T = typename R::type; using C = typename decltype(c)::type;
    if (rb % C::NRT) return hipErrorInvalidValue;                   // whole workgroups per (x block, iy)
    return launch_one<C>(xgather_row_io(R::p(src), R::p(dst), scale, M, tc, rb, ny), nrows, R::p(tw), partials, s);
  });
}
hipError_t launch_row_c2r_lognormal(int f64, int M, void* W, long long nrows, double scale, const double* Ap, const double* Bp,
                                    const void* tw, double* partials, hipStream_t s) {
  return for_rows(f64, M, hipErrorInvalidValue, [&](auto r, auto c) {
    using R = decltype(r); using T = typename R::type; using C = typename decltype(c)::type;
    LognormalIO<T, C::M> io; io.base = R::p(W); io.scale = (T)scale; io.M_of = M; io.Ap = Ap; io.Bp = Bp;
    return launch_one<C>(io, nrows, R::p(tw), partials, s);
  });
}
hipError_t launch_row_c2r_zscale(int f64, int M, void* W, long long nrows, double scale, const double* Sz, const void* tw, double* partials,
                                 hipStream_t s) {
  return for_rows(f64, M, hipErrorInvalidValue, [&](auto r, auto c) {
    using R = decltype(r); using T = typename R::type;
    ScaleZRowIO<T> io; io.base = R::p(W); io.scale = (T)scale; io.M_of = M; io.Sz = Sz;
    return launch_one<typename decltype(c)::type>(io, nrows, R::p(tw), partials, s);
  });
}
hipError_t launch_row_r2c(int f64, int M, void* W, long long nrows, const void* tw, hipStream_t s) {
  return for_rows(f64, M, hipErrorInvalidValue, [&](auto r, auto c) {
    using R = decltype(r); using T = typename R::type; using C = typename decltype(c)::type;
    PlainRowFwdIO<T> io; io.base = R::p(W); io.M_of = M;
    return tile_launch<row_r2c_kernel<C, PlainRowFwdIO<T>>>(row_tiles<C>(nrows), C::NT, fwd_lds_bytes<C>(), s, io, R::p(tw), nrows);
  });
}

hipError_t prepare_rows(int f64, int M) {
  Prepare p;
  for_rows(f64, M, 0, [&](auto r, auto c) {
    using T = typename decltype(r)::type; using C = typename decltype(c)::type;
    constexpr int lds = row_lds_bytes<C>();
    p.kernel<row_c2r_kernel<C, PlainRowIO<T>>>(lds);
    p.kernel<row_c2r_kernel<C, GatherRowIO<T>>>(lds);
    p.kernel<row_c2r_kernel<C, XGatherRowIO<T>>>(lds);
    p.kernel<row_c2r_kernel<C, LognormalIO<T, C::M>>>(lds);
    p.kernel<row_c2r_kernel<C, ScaleZRowIO<T>>>(lds);
    p.kernel<row_r2c_kernel<C, PlainRowFwdIO<T>>>(fwd_lds_bytes<C>());
    return 0;
  });
  return p.e;
}
}  // namespace rf
