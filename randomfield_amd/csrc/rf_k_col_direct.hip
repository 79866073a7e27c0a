// rf_k_col_direct.hip -- the inverse y pass of a kz-slab rank with its output stored straight into the receive buffers of the
// exchange (rf_fft.h DirectColIO / Pair2DirectColIO; DESIGN.md section 5, "direct" mode).  Same configurations and the same
// arithmetic per tile as the in-place pass (rf_k_col_plain.hip launch_col_plain): only the base pointer of the stores differs,
// chosen once per workgroup from a device table of per-destination pointers.
#include "rf_tile_launch.h"

namespace rf {
namespace {

// Tile order: xcd_tile gives XCD j the j-th eighth of the tiles, i.e. of the x planes -- with 8 ranks XCD j stores to rank j, and all
// 8 destinations (7 links + the local segment) are being written at any one time.
template <class C, class IO>
__global__ __launch_bounds__(C::NT, (col_min_waves<C, IO>())) void col_direct_kernel(IO io, const cplx<typename C::T>* __restrict__ tw, long long ntiles) {
  extern __shared__ __attribute__((aligned(16))) char rf_smem[];
  const long long tile = xcd_tile(blockIdx.x, ntiles);
  io.bind_tile(tile * C::TC);
  col_body<C, +1, IO>(io, tw, tile, rf_smem);
}

template <class C1, class IO>
__global__ __launch_bounds__(C1::NT, (col_min_waves<C1, IO>())) void col2_direct_kernel(IO io, const cplx<typename C1::T>* __restrict__ tw2, long long ntiles) {
  extern __shared__ __attribute__((aligned(16))) char rf_smem[];
  const long long tile = xcd_tile(blockIdx.x, ntiles);
  io.bind_tile(tile * C1::TC);
  col2_body<C1, +1, IO>(io, tw2, tile, rf_smem);
}

// a tile must lie inside ONE x plane (one destination): whole tiles per run of `inner` columns
template <class C> bool tiles_ok(const ColGeom& g, long long ncols) { return ncols % C::TC == 0 && pow2(g.inner) && g.inner % C::TC == 0; }

template <class C, class IO>
hipError_t launch_one(IO io, const cplx<typename C::T>* src, ColGeom g, cplx<typename C::T>* const* tab, int dest_shift, long long ncols,
                      const cplx<typename C::T>* tw, hipStream_t s) {
  if (!tiles_ok<C>(g, ncols)) return hipErrorInvalidValue;
  io.base = const_cast<cplx<typename C::T>*>(src); io.g = g; io.tab = tab; io.dest_shift = dest_shift;
  const long long ntiles = ncols / C::TC;
  return tile_launch<col_direct_kernel<C, IO>>(ntiles, C::NT, lds_of<C, IO>(), s, io, tw, ntiles);
}

template <class C1>
hipError_t launch_pair(const cplx<float>* src, ColGeom g, cplx<float>* const* tab, int dest_shift, long long ncols, const cplx<float>* tw2, hipStream_t s) {
  using IO = Pair2DirectColIO<float>;
  if (!tiles_ok<C1>(g, ncols)) return hipErrorInvalidValue;
  IO io = pair2_col_io<IO>(const_cast<cplx<float>*>(src), g);
  io.tab = tab; io.dest_shift = dest_shift;
  const long long ntiles = ncols / C1::TC;
  return tile_launch<col2_direct_kernel<C1, IO>>(ntiles, C1::NT, lds_of<C1, IO>(), s, io, tw2, ntiles);
}
}  // namespace

// (halves or whole columns: the in-place pass's own rule -- rf_select.h col_halves -- so the arithmetic per tile is the same)
hipError_t launch_col_direct(int f64, int N, const void* src, ColGeom g, void* const* tab, int dest_shift, long long ncols, const void* tw,
                             hipStream_t s) {
  if (!col_direct_supported(f64, N, g.inner)) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (for_col_halves(f64, N, g, [&](auto c) {
        e = launch_pair<typename decltype(c)::type>((const cplx<float>*)src, g, (cplx<float>* const*)tab, dest_shift, ncols, (const cplx<float>*)tw, s);
      }))
    return e;
  return with_real(f64, [&](auto r) {
    using R = decltype(r); using T = typename R::type;
    return for_col_size(N, hipErrorInvalidValue, [&](auto n) {
      constexpr int NN = decltype(n)::value;
      using C = typename ColSel<T, NN>::type;
      if (g.needs_wide(C::LMAX, C::TC, (int)sizeof(cplx<T>))) {
        if constexpr (NN >= 1024) return launch_one<C>(DirectColIO<T, true>(), R::p(src), g, R::p(tab), dest_shift, ncols, R::p(tw), s);
        return hipErrorInvalidValue;
      }
      return launch_one<C>(DirectColIO<T>(), R::p(src), g, R::p(tab), dest_shift, ncols, R::p(tw), s);
    });
  });
}

hipError_t prepare_col_direct(int f64, int N) {
  Prepare p;
  for_col_halves(f64, N, [&](auto c) { using C1 = typename decltype(c)::type; using IO = Pair2DirectColIO<float>; p.kernel<col2_direct_kernel<C1, IO>>(lds_of<C1, IO>()); });
  with_real(f64, [&](auto r) {
    using T = typename decltype(r)::type;
    return for_col_size(N, 0, [&](auto n) {
      constexpr int NN = decltype(n)::value;
      using C = typename ColSel<T, NN>::type;
      if constexpr (NN >= 1024) p.kernel<col_direct_kernel<C, DirectColIO<T, true>>>(lds_of<C, DirectColIO<T, true>>());
      p.kernel<col_direct_kernel<C, DirectColIO<T>>>(lds_of<C, DirectColIO<T>>());
      return 0;
    });
  });
  return p.e;
}
}  // namespace rf
