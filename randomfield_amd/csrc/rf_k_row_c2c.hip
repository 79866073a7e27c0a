// contiguous-axis pass of the unpacked c2c transform (transform.py:207-213): plain complex rows, both directions
#include "rf_tile_launch.h"

namespace rf {
namespace {
template <class C> constexpr int lds_bytes() { return C::LDS_BYTES > 64 ? C::LDS_BYTES : 64; }
// f(Real<T>{}, the row configuration, Size<dir>{})
template <class R, class F> R for_rows(int f64, int M, int dir, R otherwise, F&& f) {
  return with_real(f64, [&](auto r) {
    return with_dir(dir, [&](auto d) {
      return for_rowc_size(M, otherwise, [&](auto m) { return f(r, Cfg<typename RowSel<typename decltype(r)::type, decltype(m)::value>::type>{}, d); });
    });
  });
}
}  // namespace

hipError_t launch_row_c2c(int f64, int M, int dir, void* W, long long nrows, double scale, const void* tw, hipStream_t s) {
  return for_rows(f64, M, dir, hipErrorInvalidValue, [&](auto r, auto c, auto d) {
    using R = decltype(r); using T = typename R::type; using C = typename decltype(c)::type;
    ScaledRowIO<T> io; io.base = R::p(W); io.M_of = M; io.scale = (T)scale;
    return tile_launch<row_c2c_kernel<C, decltype(d)::value, ScaledRowIO<T>>>((nrows + C::NRT - 1) / C::NRT, C::NT, lds_bytes<C>(), s, io, R::p(tw), nrows);
  });
}

hipError_t prepare_row_c2c(int f64, int M, int dir) {
  return for_rows(f64, M, dir, hipSuccess, [&](auto r, auto c, auto d) {
    using C = typename decltype(c)::type;
    return tile_prepare<row_c2c_kernel<C, decltype(d)::value, ScaledRowIO<typename decltype(r)::type>>>(lds_bytes<C>());
  });
}
}  // namespace rf
