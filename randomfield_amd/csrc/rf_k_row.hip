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
// float64 rows of >= 512 complex: the exp table in the tile's spare LDS slots (rf_fft.h LognormalRowIO)
template <typename T, int MM> using LognormalIO = LognormalRowIO<T, (sizeof(T) == 8 && MM >= 512) ? 1 : 0>;

// f(Real<T>{}, the row configuration) for rows of M complex of either dtype
template <class R, class F> R for_rows(int f64, int M, R otherwise, F&& f) {
  return with_real(f64, [&](auto r) {
    return for_row_size(M, otherwise, [&](auto m) { return f(r, Cfg<typename RowSel<typename decltype(r)::type, decltype(m)::value>::type>{}); });
  });
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
    GatherRowIO<T> io; io.src = R::p(src); io.dst = R::p(dst); io.scale = (T)scale; io.M_of = M; io.nzl = nzl; io.seg_stride = seg_stride;
    return launch_one<typename decltype(c)::type>(io, nrows, R::p(tw), partials, s);
  });
}
hipError_t launch_row_c2r_xgather(int f64, int M, const void* src, void* dst, long long nrows, double scale, int tc, int rb, int ny,
                                  const void* tw, double* partials, hipStream_t s) {
  if (!pow2(tc) || !pow2(rb) || !pow2(ny) || M % tc || nrows % rb) return hipErrorInvalidValue;
  return for_rows(f64, M, hipErrorInvalidValue, [&](auto r, auto c) {
    using R = decltype(r); using T = typename R::type; using C = typename decltype(c)::type;
    if (rb % C::NRT) return hipErrorInvalidValue;                   // whole workgroups per (x block, iy)
    XGatherRowIO<T> io; io.src = R::p(src); io.dst = R::p(dst); io.scale = (T)scale; io.M_of = M;
    io.seg_shift = ilog2ll(tc); io.rb_shift = ilog2ll(rb); io.ny_shift = ilog2ll(ny);
    io.kt_stride = (long long)ny * rb * tc; io.xb_stride = (long long)(M / tc) * io.kt_stride;
    return launch_one<C>(io, nrows, R::p(tw), partials, s);
  });
}
// can the gathering z pass of rows of M complex serve tiles of tc columns and x blocks of rb rows?
bool row_c2r_xgather_ok(int f64, int M, int tc, int rb) {
  return for_rows(f64, M, false, [&](auto, auto c) { return tc > 0 && rb > 0 && rb % decltype(c)::type::NRT == 0 && M % tc == 0; });
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
long long row_c2r_tiles(int f64, int M, long long nrows) {
  return for_rows(f64, M, -1LL, [&](auto, auto c) { return row_tiles<typename decltype(c)::type>(nrows); });
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
