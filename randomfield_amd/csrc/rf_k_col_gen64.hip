// the float64 fast-generation x pass (values drawn in float32 arithmetic and widened): its own translation unit, compiled with the
// compiler's default scheduling strategy (rf_col_gen_launch.h)
#include "rf_col_gen_launch.h"

namespace rf {
namespace {
template <class V, int FIX> struct FastIo64 { using type = FastGenColIO64<FIX, V::slab, V::pot, V::halves ? 2 : 1>; };
// (length 1024 as two 512-point transforms per tile, Col2: two workgroups per CU -- DESIGN.md 3.10)
using Fast64 = FastGen<double, FastIo64>;
}  // namespace

hipError_t launch_col_fastgen64(int N, const FastVariant& v, void* W, ColGeom g, long long ncols, const FastGenParams& gp, int kz0, int nzl, const void* tw,
                                hipStream_t s, hipEvent_t after_repair, int x0, int x1, void* pot, void* fixbuf) {
  using R = Real<double>;
  return Fast64::launch(N, v, FastArgs<double>{gp, R::p(W), g, ncols, kz0, nzl, R::p(tw), s, after_repair, x0, x1, R::p(pot), R::p(fixbuf)});
}

hipError_t prepare_col_fastgen64(int N) { return Fast64::prepare(N); }

}  // namespace rf
