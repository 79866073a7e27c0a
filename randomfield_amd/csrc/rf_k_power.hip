// the binned power spectrum estimator of rf_measure_power (rf_core.h power_cell): one sweep of the half spectrum into per-workgroup
// histograms, one fixed-order reduction of those.  No floating-point atomics anywhere: the same plan, data and edges give the same
// bits on every call.
#include "rf_kernels.h"
#include "rf_launch.h"

namespace rf {
namespace {

// Rows (ix, iy) of the half spectrum as derivative_kernel walks them: blockDim.x threads along kz, blockDim.y rows per workgroup.  Every
// wave owns a histogram in LDS ([waves][nbins] of sum_k, sum_p, count behind the nbins + 1 squared edges).  Per step of 64 cells the
// bins of a wave are reduced in one of two fixed-order ways.  Rows of at least a wave (blockDim.x >= 64) whose kz2 table does not
// decrease: equal bins are runs of neighbouring lanes, a segmented scan sums every run and the runs' last lanes add to the wave's
// histogram together (with min(shape) / 2 linear bins a step near the kz axis meets ~40 bins: a loop over bins, 30 cross-lane
// operations each, ran the 1024^3 sweep at 83 ms).  Otherwise (several short rows in a wave) the wave loops while binned lanes remain:
// the lowest remaining lane's bin is taken, its members are reduced by a fixed shuffle tree (the others contribute an exact 0) and
// lane 0 adds the three sums.  At the end the waves' histograms are summed in wave order into row blockIdx.x of the three
// partial planes [gridDim.x][nbins]; every bin is written, so the planes need no clearing.
// Every thread of a workgroup runs the same number of row and kz steps (lanes without a cell carry bin -1): the shuffles and
// ballots always see whole waves.
template <typename T>
__global__ __launch_bounds__(256) void power_sweep_kernel(const cplx<T>* __restrict__ S, PowerParams gp, const double* __restrict__ e2_dev,
                                                          unsigned nrows, unsigned long long* __restrict__ pc, double* __restrict__ pk,
                                                          double* __restrict__ pp) {
  extern __shared__ double power_lds[];
  const int nb = gp.nbins;
  const int nthreads = blockDim.x * blockDim.y, tid = threadIdx.y * blockDim.x + threadIdx.x;
  const int nw = nthreads >> 6, wave = tid >> 6, lane = tid & 63;
  double* e2 = power_lds;                                   // [nb + 1]
  double* hk = e2 + (nb + 1);                               // [nw][nb]
  double* hp = hk + nw * nb;                                // [nw][nb]
  unsigned long long* hc = reinterpret_cast<unsigned long long*>(hp + nw * nb);   // [nw][nb]
  for (int i = tid; i <= nb; i += nthreads) e2[i] = e2_dev[i];
  for (int i = tid; i < nw * nb; i += nthreads) { hk[i] = 0.0; hp[i] = 0.0; hc[i] = 0ull; }
  __syncthreads();
  const int nzh = gp.nz / 2 + 1;
  const bool runs = gp.kz_sorted && blockDim.x >= 64;
  double* wk_h = hk + wave * nb;
  double* wp_h = hp + wave * nb;
  unsigned long long* wc_h = hc + wave * nb;
  for (unsigned long long r0 = (unsigned long long)blockIdx.x * blockDim.y; r0 < nrows; r0 += (unsigned long long)gridDim.x * blockDim.y) {
    const unsigned long long rr = r0 + threadIdx.y;
    const bool row_ok = rr < nrows;
    const unsigned row = row_ok ? (unsigned)rr : 0u, ix = row / (unsigned)gp.ny, iy = row - ix * (unsigned)gp.ny;
    for (int iz0 = 0; iz0 < nzh; iz0 += blockDim.x) {
      const int iz = iz0 + threadIdx.x;
      int b = -1, w = 0;
      double wk = 0.0, wp = 0.0;
      if (row_ok && iz < nzh) b = power_cell<T>(gp, e2, power_load<T>(gp, S, (int)ix, (int)iy, iz), (int)ix, (int)iy, iz, w, wk, wp);
      if (runs) {
        // the wave's 64 cells are consecutive kz of one row and their bins do not decrease: equal bins are runs of neighbouring lanes.
        // A segmented inclusive scan (six fixed steps, whatever the number of bins) leaves every run's sums in its last lane, and the
        // last lanes -- one per bin -- add them to the wave's histogram in one step
        double sk = wk, sp = wp;
        int sc = w;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int bo = __shfl_up(b, off);
          const double tk = __shfl_up(sk, off), tp = __shfl_up(sp, off);
          const int tc = __shfl_up(sc, off);
          if (lane >= off && bo == b) { sk += tk; sp += tp; sc += tc; }
        }
        const int bn = __shfl_down(b, 1);
        if (b >= 0 && (lane == 63 || bn != b)) { wk_h[b] += sk; wp_h[b] += sp; wc_h[b] += (unsigned long long)sc; }
        continue;
      }
      unsigned long long rem = __ballot(b >= 0);
      while (rem) {
        const int bb = __shfl(b, __ffsll((long long)rem) - 1);
        const bool mine = b == bb;
        double sk = mine ? wk : 0.0, sp = mine ? wp : 0.0;
        int sc = mine ? w : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { sk += __shfl_down(sk, off); sp += __shfl_down(sp, off); sc += __shfl_down(sc, off); }
        if (lane == 0) { wk_h[bb] += sk; wp_h[bb] += sp; wc_h[bb] += (unsigned long long)sc; }
        rem &= ~__ballot(mine);
      }
    }
  }
  __syncthreads();
  const long long base = (long long)blockIdx.x * nb;
  for (int i = tid; i < nb; i += nthreads) {
    double k = 0.0, q = 0.0;
    unsigned long long c = 0ull;
    for (int v = 0; v < nw; ++v) { k += hk[v * nb + i]; q += hp[v * nb + i]; c += hc[v * nb + i]; }
    pk[base + i] = k; pp[base + i] = q; pc[base + i] = c;
  }
}

// out = the nwg rows of the partial planes summed in row order: 16 bins x 16 chunks of rows per workgroup, the chunks of a bin combined
// in chunk order.  out: [count nbins][sum_k nbins][sum_p nbins]
__global__ __launch_bounds__(256) void power_reduce_kernel(const unsigned long long* __restrict__ pc, const double* __restrict__ pk,
                                                           const double* __restrict__ pp, int nwg, int nb, unsigned long long* __restrict__ oc,
                                                           double* __restrict__ ok, double* __restrict__ op) {
  __shared__ double rk[16][17], rp[16][17];
  __shared__ unsigned long long rc[16][17];
  const int bl = threadIdx.x & 15, ch = threadIdx.x >> 4, b = blockIdx.x * 16 + bl;
  const int per = (nwg + 15) / 16, lo = ch * per, hi = lo + per < nwg ? lo + per : nwg;
  double k = 0.0, q = 0.0;
  unsigned long long c = 0ull;
  if (b < nb) {
#pragma unroll 8
    for (int g = lo; g < hi; ++g) { const long long i = (long long)g * nb + b; k += pk[i]; q += pp[i]; c += pc[i]; }
  }
  rk[ch][bl] = k; rp[ch][bl] = q; rc[ch][bl] = c;
  __syncthreads();
  if (ch == 0 && b < nb) {
    k = 0.0; q = 0.0; c = 0ull;
    for (int v = 0; v < 16; ++v) { k += rk[v][bl]; q += rp[v][bl]; c += rc[v][bl]; }
    ok[b] = k; op[b] = q; oc[b] = c;
  }
}

}  // namespace

PowerLaunch power_launch_shape(int nx, int ny, int nz, int nbins) {
  PowerLaunch L;
  // a wave's histogram takes 24 bytes per bin: four waves per workgroup up to 512 bins, two above, stay inside 64 KB of LDS
  const int nthreads = nbins <= 512 ? 256 : 128;
  const int nzh = nz / 2 + 1;
  int tx = 1;
  while (tx < nthreads && tx < nzh) tx <<= 1;
  L.tx = tx;
  L.ty = nthreads / tx;
  const long long nrows = (long long)nx * ny, nblk = (nrows + L.ty - 1) / L.ty;
  const long long cap = nbins <= 128 ? 2048 : 1024;        // workgroups: rows of the partial planes (<= 2^20 words per plane); more rows than cap * ty: tests/test_gpu_at_scale.py
  L.grid = (unsigned)(nblk < cap ? (nblk < 1 ? 1 : nblk) : cap);
  L.lds = (size_t)((nbins + 1) + 3 * (nthreads / 64) * nbins) * 8;
  return L;
}

hipError_t launch_power(int f64, const void* S, const PowerParams& gp, const double* e2_dev, unsigned long long* partials, long long plane_words,
                        unsigned long long* out, hipStream_t s) {
  const long long nrows = (long long)gp.nx * gp.ny;
  if (nrows <= 0 || nrows > 0x7fffffffLL || gp.nbins < 1 || gp.nbins > 1024 || (gp.nz & 1)) return hipErrorInvalidValue;
  const PowerLaunch L = power_launch_shape(gp.nx, gp.ny, gp.nz, gp.nbins);
  if ((long long)L.grid * gp.nbins > plane_words || L.lds > 65536) return hipErrorInvalidValue;
  unsigned long long* pc = partials;
  double* pk = reinterpret_cast<double*>(partials + plane_words);
  double* pp = reinterpret_cast<double*>(partials + 2 * plane_words);
  if (f64) hipLaunchKernelGGL(power_sweep_kernel<double>, dim3(L.grid), dim3(L.tx, L.ty), L.lds, s, (const cplx<double>*)S, gp, e2_dev, (unsigned)nrows, pc, pk, pp);
  else hipLaunchKernelGGL(power_sweep_kernel<float>, dim3(L.grid), dim3(L.tx, L.ty), L.lds, s, (const cplx<float>*)S, gp, e2_dev, (unsigned)nrows, pc, pk, pp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(power_reduce_kernel, dim3((unsigned)((gp.nbins + 15) / 16)), dim3(256), 0, s, pc, pk, pp, (int)L.grid, gp.nbins, out,
                     reinterpret_cast<double*>(out + gp.nbins), reinterpret_cast<double*>(out + 2 * gp.nbins));
  return hipGetLastError();
}

}  // namespace rf
