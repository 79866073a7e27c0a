// the float64 fast-generation x pass (values drawn in float32 arithmetic and widened): its own translation unit, compiled with the
// compiler's default scheduling strategy (rf_col_gen_launch.h)
#include "rf_col_gen_launch.h"

namespace rf {

hipError_t launch_col_fastgen64(int N, const FastVariant& v, void* W, ColGeom g, long long ncols, const FastGenParams& gp, int kz0, int nzl, const void* tw,
                                hipStream_t s, hipEvent_t after_repair, int x0, int x1, void* pot, void* fixbuf) {
  using R = Real<double>;
  return fastgen_launch<double>(N, v, FastArgs<double>{{gp, R::p(W), g, kz0, nzl, x0, x1, R::p(pot), R::p(fixbuf)}, ncols, R::p(tw), s, after_repair});
}

hipError_t prepare_col_fastgen64(int N) { return fastgen_prepare<double>(N); }

}  // namespace rf
