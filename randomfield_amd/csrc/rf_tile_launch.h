// rf_tile_launch.h -- the one launch step of the tiled power-of-two kernels (included by the rf_k_*.hip launchers only).
// A launcher = its family's argument checks + one tile_launch<kernel>(...); what plan creation prepares = tile_prepare<kernel>(lds) over
// the same kernels, enumerated (prepare_packed_kernels / prepare_c2c_kernels, rf_launch.h).  Which kernel: rf_select.h.
#pragma once
#include "rf_kernels.h"
#include "rf_launch.h"
#include "rf_select.h"

namespace rf {

// what each translation unit prepares for plan creation: every kernel its launchers can choose for (dtype, length)
hipError_t prepare_col_plain(int f64, int N, int dir, bool inverse_forms);   // rf_k_col_plain.hip (inverse_forms: + out of place, + accumulating)
hipError_t prepare_col_direct(int f64, int N);                               // rf_k_col_direct.hip
hipError_t prepare_col_gen(int f64, int N);                                  // rf_k_col_gen.hip: the exact pass and every fast variant
hipError_t prepare_col_fastgen64(int N);                                     // rf_k_col_gen64.hip
hipError_t prepare_rows(int f64, int M);                                     // rf_k_row.hip: every c2r form and the r2c pass
hipError_t prepare_row_c2c(int f64, int M, int dir);                         // rf_k_row_c2c.hip
hipError_t prepare_yz_merged(int f64, int ny, int M);                        // rf_k_yz.hip

namespace {

// Kernels with more than 64 KB of dynamic LDS need their function attribute set once per device, and never inside a graph capture:
// plan creation calls this for every kernel the plan can launch.  (One latch per kernel instantiation.)
template <auto K>
hipError_t tile_prepare(int lds_bytes) {
  static LdsAttrLatch latch;
  return latch.ensure((const void*)K, lds_bytes);
}

// (the launch keeps its own `ensure`: a kernel that plan creation missed still gets its attribute, as before)
template <auto K, class... A>
hipError_t tile_launch(long long grid, int nt, int lds_bytes, hipStream_t s, A... args) {
  if (hipError_t e = tile_prepare<K>(lds_bytes); e != hipSuccess) return e;
  hipLaunchKernelGGL(K, dim3((unsigned)grid), dim3(nt), lds_bytes, s, args...);
  return hipGetLastError();
}

inline bool pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }
// dynamic LDS of a strided pass: the tile and its twiddles + the IO's own tables -- and never less than the NT / 64 doubles through
// which an IO with a finish() step (AccColIO) adds up its waves at the start of the workgroup's LDS (rf_kernels.h col_body): the
// one-pass configurations (lengths 8 and 16) have no tile, and with no LDS at all the partial sums were dropped -- every tile's
// Parseval partial, and so the sigma of rf_realise_lognormal, came out 0 on plans with ny = 8 or 16
template <class IO, class = void> struct io_finish_bytes { static constexpr int of(int) { return 0; } };
template <class IO> struct io_finish_bytes<IO, typename std::enable_if<IO::HAS_FINISH>::type> {
  static constexpr int of(int nthreads) { return nthreads / 64 * (int)sizeof(double); }
};
template <class C, class IO> constexpr int lds_of() {
  constexpr int pass = C::LDS_BYTES + IO::LDS_EXTRA, red = io_finish_bytes<IO>::of(C::NT);
  return pass > red ? pass : red;
}

// a run of preparations that stops at the first failure
struct Prepare {
  hipError_t e = hipSuccess;
  template <auto K> void kernel(int lds_bytes) { if (e == hipSuccess) e = tile_prepare<K>(lds_bytes); }
};

}  // namespace
}  // namespace rf
