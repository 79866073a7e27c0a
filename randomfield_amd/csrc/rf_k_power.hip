// the binned estimators of rf_measure_power and rf_measure_multipoles (rf_core.h bin_cell: power_cell with two float64 sums per bin --
// sum_k, sum_p -- or multipole_cell with four -- sum_k and the moments m0, m2, m4 of mu^2 -- and the count): one sweep of the half
// spectrum into per-workgroup histograms, one fixed-order reduction of those.  No floating-point atomics anywhere: the same plan, data,
// edges and tables give the same bits on every call.
#include "rf_kernels.h"
#include "rf_launch.h"

namespace rf {
namespace {

// The workgroup's LDS, [nb + 1 squared edges][NS][nw][nb] float64 sums][nw][nb] counts]: every wave owns a histogram.
template <int NS>
struct BinHist {
  int nb, nthreads, tid, nw, lane, js;
  double* e2;                 // [nb + 1]
  double* hd;                 // [NS][nw][nb]
  unsigned long long* hc;     // [nw][nb]
  double* wd;                 // sum j of this wave's bin b: wd[j * js + b]
  unsigned long long* wc;
  // (the bin is added to wd first: written as wd[j * js + b], the compiler keeps the NS addresses wd + j * js in registers of their own
  // through the whole sweep)
  __device__ void add(int b, const double (&s)[NS], int c) const {
#pragma unroll
    for (int j = 0; j < NS; ++j) (wd + b)[j * js] += s[j];
    wc[b] += (unsigned long long)c;
  }
};

// edges into LDS, histograms cleared
template <int NS>
__device__ BinHist<NS> bin_prologue(double* lds, const double* __restrict__ e2_dev, int nb) {
  BinHist<NS> h;
  h.nb = nb;
  h.nthreads = blockDim.x * blockDim.y;
  h.tid = threadIdx.y * blockDim.x + threadIdx.x;
  h.nw = h.nthreads >> 6;
  h.lane = h.tid & 63;
  h.js = h.nw * nb;
  h.e2 = lds;
  h.hd = h.e2 + (nb + 1);
  h.hc = reinterpret_cast<unsigned long long*>(h.hd + NS * h.js);
  for (int i = h.tid; i <= nb; i += h.nthreads) h.e2[i] = e2_dev[i];
  for (int i = h.tid; i < NS * h.js; i += h.nthreads) h.hd[i] = 0.0;
  for (int i = h.tid; i < h.js; i += h.nthreads) h.hc[i] = 0ull;
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(h.tid >> 6);      // the same in every lane of a wave: said so, wd and wc stay in scalar registers
  h.wd = h.hd + wave * nb;
  h.wc = h.hc + wave * nb;
  return h;
}

// the waves' histograms summed in wave order into row blockIdx.x of the partial planes [count][NS sums], each [gridDim.x][nb]; every
// bin is written, so the planes need no clearing
template <int NS>
__device__ void bin_epilogue(const BinHist<NS>& h, unsigned long long* __restrict__ pc, double* __restrict__ pd, long long plane_words) {
  __syncthreads();
  const int nb = h.nb;
  const long long base = (long long)blockIdx.x * nb;
  for (int i = h.tid; i < nb; i += h.nthreads) {
    double s[NS] = {};
    unsigned long long c = 0ull;
    for (int v = 0; v < h.nw; ++v) {
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] += h.hd[j * h.js + v * nb + i];
      c += h.hc[v * nb + i];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) pd[j * plane_words + base + i] = s[j];
    pc[base + i] = c;
  }
}

// Segmented inclusive scan over the wave, keyed by b (equal keys are runs of neighbouring lanes): six fixed steps, whatever the number
// of bins, leave every run's sums in its last lane.
template <int NS>
__device__ void bin_scan(int lane, int b, double (&s)[NS], int& sc) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int bo = __shfl_up(b, off);
    double t[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) t[j] = __shfl_up(s[j], off);
    const int tc = __shfl_up(sc, off);
    if (lane >= off && bo == b) {
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] += t[j];
      sc += tc;
    }
  }
}

// Rows (ix, iy) of the half spectrum as derivative_kernel walks them: blockDim.x threads along kz, blockDim.y rows per workgroup, a
// grid-stride loop over the rows.  Per step of 64 cells the bins of a wave are reduced in one of two fixed-order ways.  Rows of at
// least a wave (blockDim.x >= 64) whose kz2 table does not decrease: the wave's 64 cells are consecutive kz of one row, equal bins are
// runs of neighbouring lanes, bin_scan sums every run and the runs' last lanes -- one per bin -- add to the wave's histogram together
// (with min(shape) / 2 linear bins a step near the kz axis meets ~40 bins: a loop over bins, 30 cross-lane operations each, ran the
// 1024^3 sweep at 83 ms).  Otherwise (several short rows in a wave) the wave loops while binned lanes remain: the lowest remaining
// lane's bin is taken, its members are reduced by a fixed shuffle tree (the others contribute an exact 0) and lane 0 adds the sums.
// Every thread of a workgroup runs the same number of row and kz steps (lanes without a cell carry bin -1): the shuffles and ballots
// always see whole waves.
// The compensation tables of the multipoles are read where the k^2 tables are, through multipole_cell's global loads: cx and cy are
// one value per row and cz is nz/2 + 1 values that every row reads again (cache resident); at 1024 bins the histograms leave no LDS
// for them.
template <typename T, typename P>
__global__ __launch_bounds__(256) void bin_sweep_kernel(const cplx<T>* __restrict__ S, P g, const double* __restrict__ e2_dev, unsigned nrows,
                                                        unsigned long long* __restrict__ pc, double* __restrict__ pd, long long plane_words) {
  constexpr int NS = BinSums<P>::N;
  extern __shared__ double bin_lds[];
  const PowerParams& gp = bin_geom(g);
  const BinHist<NS> h = bin_prologue<NS>(bin_lds, e2_dev, gp.nbins);
  const int nzh = gp.nz / 2 + 1, lane = h.lane;
  const bool runs = gp.kz_sorted && blockDim.x >= 64;
  for (unsigned long long r0 = (unsigned long long)blockIdx.x * blockDim.y; r0 < nrows; r0 += (unsigned long long)gridDim.x * blockDim.y) {
    const unsigned long long rr = r0 + threadIdx.y;
    const bool row_ok = rr < nrows;
    const unsigned row = row_ok ? (unsigned)rr : 0u, ix = row / (unsigned)gp.ny, iy = row - ix * (unsigned)gp.ny;
    for (int iz0 = 0; iz0 < nzh; iz0 += blockDim.x) {
      const int iz = iz0 + threadIdx.x;
      int b = -1, w = 0;
      double d[NS] = {};
      if (row_ok && iz < nzh) b = bin_cell<T>(g, h.e2, power_load<T>(gp, S, (int)ix, (int)iy, iz), (int)ix, (int)iy, iz, w, d);
      if (runs) {
        bin_scan<NS>(lane, b, d, w);
        const int bn = __shfl_down(b, 1);
        if (b >= 0 && (lane == 63 || bn != b)) h.add(b, d, w);
        continue;
      }
      unsigned long long rem = __ballot(b >= 0);
      while (rem) {
        const int bb = __shfl(b, __ffsll((long long)rem) - 1);
        const bool mine = b == bb;
        double s[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j] = mine ? d[j] : 0.0;
        int sc = mine ? w : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
          for (int j = 0; j < NS; ++j) s[j] += __shfl_down(s[j], off);
          sc += __shfl_down(sc, off);
        }
        if (lane == 0) h.add(bb, s, sc);
        rem &= ~__ballot(mine);
      }
    }
  }
  bin_epilogue<NS>(h, pc, pd, plane_words);
}

// The same sweep for rows of at least 64 * CELLS cells with a kz2 table that does not decrease (bin_launch_shape: `cells`): a lane
// takes CELLS consecutive cells of the row, so that CELLS loads are in flight per lane and one scan serves 64 * CELLS cells.  The
// bins of a lane's cells form runs.  A run strictly inside the lane -- neither its first nor its last -- belongs to no other lane and
// is added to the histogram by the lane itself.  The last run (the only one, if the bins do not change) goes into the segmented scan
// keyed by its bin: a lane whose bins change starts a key larger than every key before it, so equal keys are still neighbouring lanes.
// The first run of a lane whose bins change ends the run of the lanes before it: the lane adds the scan's value of the lane before
// (if that lane's key is this bin) to its own part and adds the total to the histogram; a lane adds its scanned run itself only when
// the next lane's first bin differs.  No two lanes add to one bin in the same instruction, and every order is fixed.  Dropped cells
// carry bin -1 and zeros: -1 is never added, and a row's valid cells are one block, so the runs of valid bins stay contiguous.
// A wave without a single binned cell in a step skips the step (decided by a ballot: whole waves).
template <typename T, typename P, int CELLS>
__global__ __launch_bounds__(256) void bin_sweep_cells_kernel(const cplx<T>* __restrict__ S, P g, const double* __restrict__ e2_dev, unsigned nrows,
                                                              unsigned long long* __restrict__ pc, double* __restrict__ pd, long long plane_words) {
  constexpr int NS = BinSums<P>::N;
  extern __shared__ double bin_lds[];
  const PowerParams& gp = bin_geom(g);
  const BinHist<NS> h = bin_prologue<NS>(bin_lds, e2_dev, gp.nbins);
  const int nzh = gp.nz / 2 + 1, lane = h.lane;
  for (unsigned long long r0 = (unsigned long long)blockIdx.x * blockDim.y; r0 < nrows; r0 += (unsigned long long)gridDim.x * blockDim.y) {
    const unsigned long long rr = r0 + threadIdx.y;
    const bool row_ok = rr < nrows;
    const unsigned row = row_ok ? (unsigned)rr : 0u, ix = row / (unsigned)gp.ny, iy = row - ix * (unsigned)gp.ny;
    for (int iz0 = 0; iz0 < nzh; iz0 += blockDim.x * CELLS) {
      const int izb = iz0 + threadIdx.x * CELLS;
      cplx<T> v[CELLS];
#pragma unroll
      for (int c = 0; c < CELLS; ++c)
        if (row_ok && izb + c < nzh) v[c] = power_load<T>(gp, S, (int)ix, (int)iy, izb + c);
      // the lane's runs: `head` is the first run once the bins have changed (hb = -2: they have not), `cur` the run being summed
      int b0 = -1, hb = -2, hw = 0, cb = -1, cw = 0;
      double hs[NS] = {}, cs[NS] = {};
      bool any = false;
#pragma unroll
      for (int c = 0; c < CELLS; ++c) {
        int b = -1, w = 0;
        double d[NS] = {};
        if (row_ok && izb + c < nzh) b = bin_cell<T>(g, h.e2, v[c], (int)ix, (int)iy, izb + c, w, d);
        any = any || b >= 0;
        if (c == 0) {
          b0 = b; cb = b; cw = w;
#pragma unroll
          for (int j = 0; j < NS; ++j) cs[j] = d[j];
        } else if (b == cb) {
          cw += w;
#pragma unroll
          for (int j = 0; j < NS; ++j) cs[j] += d[j];
        } else {
          if (hb == -2) {                      // the first run ends: kept for after the scan
            hb = cb; hw = cw;
#pragma unroll
            for (int j = 0; j < NS; ++j) hs[j] = cs[j];
          } else if (cb >= 0) {                // a run strictly inside the lane: no other lane holds this bin
            h.add(cb, cs, cw);
          }
          cb = b; cw = w;
#pragma unroll
          for (int j = 0; j < NS; ++j) cs[j] = d[j];
        }
      }
      if (__ballot(any) == 0ull) continue;
      bin_scan<NS>(lane, cb, cs, cw);          // the lanes' last runs, keyed by their bins
      const int pb = __shfl_up(cb, 1), pw = __shfl_up(cw, 1);
      double ps[NS];
#pragma unroll
      for (int j = 0; j < NS; ++j) ps[j] = __shfl_up(cs[j], 1);
      const int nb0 = __shfl_down(b0, 1);
      if (hb >= 0) {                           // the first run of a lane whose bins change: the run of the lanes before ends here
        if (lane > 0 && pb == hb) {
          hw += pw;
#pragma unroll
          for (int j = 0; j < NS; ++j) hs[j] += ps[j];
        }
        h.add(hb, hs, hw);
      }
      if (cb >= 0 && (lane == 63 || nb0 != cb)) h.add(cb, cs, cw);
    }
  }
  bin_epilogue<NS>(h, pc, pd, plane_words);
}

// out = the nwg rows of the partial planes summed in row order: 16 bins x 16 chunks of rows per workgroup, the chunks of a bin combined
// in chunk order.  oc: [count nbins], od: [NS sums][nbins]
template <int NS>
__global__ __launch_bounds__(256) void bin_reduce_kernel(const unsigned long long* __restrict__ pc, const double* __restrict__ pd, long long plane_words,
                                                         int nwg, int nb, unsigned long long* __restrict__ oc, double* __restrict__ od) {
  __shared__ double rd[NS][16][17];
  __shared__ unsigned long long rc[16][17];
  const int bl = threadIdx.x & 15, ch = threadIdx.x >> 4, b = blockIdx.x * 16 + bl;
  const int per = (nwg + 15) / 16, lo = ch * per, hi = lo + per < nwg ? lo + per : nwg;
  double s[NS] = {};
  unsigned long long c = 0ull;
  if (b < nb) {
#pragma unroll 16 / NS
    for (int g = lo; g < hi; ++g) {
      const long long i = (long long)g * nb + b;
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] += pd[j * plane_words + i];
      c += pc[i];
    }
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) rd[j][ch][bl] = s[j];
  rc[ch][bl] = c;
  __syncthreads();
  if (ch == 0 && b < nb) {
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = 0.0;
    c = 0ull;
    for (int v = 0; v < 16; ++v) {
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] += rd[j][v][bl];
      c += rc[v][bl];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) od[j * nb + b] = s[j];
    oc[b] = c;
  }
}

template <typename P>
hipError_t launch_bins_impl(int f64, const void* S, const P& g, const double* e2_dev, unsigned long long* partials, long long plane_words,
                            unsigned long long* out, hipStream_t s) {
  constexpr int NS = BinSums<P>::N;
  constexpr BinTable T = bin_table<P>();
  const PowerParams& gp = bin_geom(g);
  const long long nrows = (long long)gp.nx * gp.ny;
  if (nrows <= 0 || nrows > 0x7fffffffLL || gp.nbins < 1 || gp.nbins > 1024 || (gp.nz & 1)) return hipErrorInvalidValue;
  const BinLaunch L = bin_launch_shape(T, gp.nx, gp.ny, gp.nz, gp.nbins);
  if ((long long)L.grid * gp.nbins > plane_words || L.lds > 65536) return hipErrorInvalidValue;
  unsigned long long* pc = partials;
  double* pd = reinterpret_cast<double*>(partials + plane_words);
  const dim3 grid(L.grid), block(L.tx, L.ty);
  const bool cells = L.cells == 4 && gp.kz_sorted && L.tx >= 64;
  if constexpr (T.cells4) {                    // (an estimator that never takes four cells per lane has no such kernel)
    if (cells) {
      if (f64) hipLaunchKernelGGL((bin_sweep_cells_kernel<double, P, 4>), grid, block, L.lds, s, (const cplx<double>*)S, g, e2_dev, (unsigned)nrows, pc, pd, plane_words);
      else hipLaunchKernelGGL((bin_sweep_cells_kernel<float, P, 4>), grid, block, L.lds, s, (const cplx<float>*)S, g, e2_dev, (unsigned)nrows, pc, pd, plane_words);
    }
  }
  if (!cells) {
    if (f64) hipLaunchKernelGGL((bin_sweep_kernel<double, P>), grid, block, L.lds, s, (const cplx<double>*)S, g, e2_dev, (unsigned)nrows, pc, pd, plane_words);
    else hipLaunchKernelGGL((bin_sweep_kernel<float, P>), grid, block, L.lds, s, (const cplx<float>*)S, g, e2_dev, (unsigned)nrows, pc, pd, plane_words);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bin_reduce_kernel<NS>, dim3((unsigned)((gp.nbins + 15) / 16)), dim3(256), 0, s, pc, pd, plane_words, (int)L.grid, gp.nbins, out,
                     reinterpret_cast<double*>(out + gp.nbins));
  return hipGetLastError();
}

}  // namespace

BinLaunch bin_launch_shape(const BinTable& t, int nx, int ny, int nz, int nbins) {
  BinLaunch L;
  // a wave's histogram takes 8 t.planes bytes per bin behind the nbins + 1 edges (24: the power spectrum, 40: the multipoles, 57 KB at
  // one wave of 1024 bins): the table's thresholds keep four, two and one wave per workgroup inside 64 KB of LDS
  const int nthreads = nbins <= t.bins256 ? 256 : (nbins <= t.bins128 ? 128 : 64);
  const int nzh = nz / 2 + 1;
  // rows of at least 256 cells: four cells per lane (bin_sweep_cells_kernel, if kz2 is sorted), threads along kz for a quarter of the row
  L.cells = t.cells4 && nzh >= 256 ? 4 : 1;
  const int span = (nzh + L.cells - 1) / L.cells;
  int tx = 1;
  while (tx < nthreads && tx < span) tx <<= 1;
  L.tx = tx;
  L.ty = nthreads / tx;
  const long long nrows = (long long)nx * ny, nblk = (nrows + L.ty - 1) / L.ty;
  const long long cap = nbins <= 128 ? 2048 : 1024;        // workgroups: rows of the partial planes (<= 2^20 words per plane); more rows than cap * ty: tests/test_gpu_at_scale.py
  L.grid = (unsigned)(nblk < cap ? (nblk < 1 ? 1 : nblk) : cap);
  L.lds = (size_t)((nbins + 1) + t.planes * (nthreads / 64) * nbins) * 8;
  return L;
}

hipError_t launch_bins(int f64, const void* S, const PowerParams& g, const double* e2_dev, unsigned long long* partials, long long plane_words,
                       unsigned long long* out, hipStream_t s) {
  return launch_bins_impl(f64, S, g, e2_dev, partials, plane_words, out, s);
}

hipError_t launch_bins(int f64, const void* S, const MultipoleParams& g, const double* e2_dev, unsigned long long* partials, long long plane_words,
                       unsigned long long* out, hipStream_t s) {
  if (g.los < 0 || g.los > 2) return hipErrorInvalidValue;
  return launch_bins_impl(f64, S, g, e2_dev, partials, plane_words, out, s);
}

}  // namespace rf
