// the power spectrum multipoles of rf_measure_multipoles (rf_core.h multipole_cell): power_sweep_kernel's scheme (rf_k_power.hip) with
// four float64 sums per bin -- sum_k and the moments m0, m2, m4 of mu^2 -- and the count.  One sweep of the half spectrum into
// per-workgroup histograms, one fixed-order reduction of those.  No floating-point atomics anywhere: the same plan, data, edges and
// tables give the same bits on every call.
#include "rf_kernels.h"
#include "rf_launch.h"

namespace rf {
namespace {

constexpr int NS = MULTIPOLE_PLANES - 1;          // float64 sums per bin: sum_k, m0, m2, m4

// Rows (ix, iy) of the half spectrum: blockDim.x threads along kz, blockDim.y rows per workgroup, a grid-stride loop over the rows.
// Every wave owns a histogram in LDS ([NS][waves][nbins] float64 and [waves][nbins] counts behind the nbins + 1 squared edges).  Per step
// of 64 cells the bins of a wave are reduced as in power_sweep_kernel: rows of at least a wave whose kz2 table does not decrease take
// the segmented inclusive scan (equal bins are runs of neighbouring lanes; six fixed steps, the runs' last lanes add to the histogram
// together); otherwise the wave loops over the bins present, lowest remaining lane first, a fixed shuffle tree per bin and lane 0 adds.
// At the end the waves' histograms are summed in wave order into row blockIdx.x of the partial planes [gridDim.x][nbins]; every bin is
// written, so the planes need no clearing.  Every thread of a workgroup runs the same number of row and kz steps (lanes without a cell
// carry bin -1): the shuffles and ballots always see whole waves.
// The compensation tables are read where the k^2 tables are, through multipole_cell's global loads: cx and cy are one value per row and
// cz is nz/2 + 1 values that every row reads again (cache resident); at 1024 bins the histograms leave no LDS for them.
template <typename T>
__global__ __launch_bounds__(256) void multipole_sweep_kernel(const cplx<T>* __restrict__ S, MultipoleParams gm, const double* __restrict__ e2_dev,
                                                              unsigned nrows, unsigned long long* __restrict__ pc, double* __restrict__ pd,
                                                              long long plane_words) {
  extern __shared__ double multipole_lds[];
  const int nb = gm.p.nbins;
  const int nthreads = blockDim.x * blockDim.y, tid = threadIdx.y * blockDim.x + threadIdx.x;
  const int nw = nthreads >> 6, wave = tid >> 6, lane = tid & 63;
  double* e2 = multipole_lds;                               // [nb + 1]
  double* hd = e2 + (nb + 1);                               // [NS][nw][nb]
  unsigned long long* hc = reinterpret_cast<unsigned long long*>(hd + NS * nw * nb);   // [nw][nb]
  for (int i = tid; i <= nb; i += nthreads) e2[i] = e2_dev[i];
  for (int i = tid; i < NS * nw * nb; i += nthreads) hd[i] = 0.0;
  for (int i = tid; i < nw * nb; i += nthreads) hc[i] = 0ull;
  __syncthreads();
  const int nzh = gm.p.nz / 2 + 1;
  const bool runs = gm.p.kz_sorted && blockDim.x >= 64;
  double* wd_h = hd + wave * nb;                            // sum j of this wave: wd_h[j * nw * nb + bin]
  const int js = nw * nb;
  unsigned long long* wc_h = hc + wave * nb;
  for (unsigned long long r0 = (unsigned long long)blockIdx.x * blockDim.y; r0 < nrows; r0 += (unsigned long long)gridDim.x * blockDim.y) {
    const unsigned long long rr = r0 + threadIdx.y;
    const bool row_ok = rr < nrows;
    const unsigned row = row_ok ? (unsigned)rr : 0u, ix = row / (unsigned)gm.p.ny, iy = row - ix * (unsigned)gm.p.ny;
    for (int iz0 = 0; iz0 < nzh; iz0 += blockDim.x) {
      const int iz = iz0 + threadIdx.x;
      int b = -1, w = 0;
      double d[NS] = {0.0, 0.0, 0.0, 0.0};
      if (row_ok && iz < nzh) {
        double m[3];
        b = multipole_cell<T>(gm, e2, power_load<T>(gm.p, S, (int)ix, (int)iy, iz), (int)ix, (int)iy, iz, w, d[0], m);
        d[1] = m[0]; d[2] = m[1]; d[3] = m[2];
      }
      if (runs) {
        double s[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j] = d[j];
        int sc = w;
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
        const int bn = __shfl_down(b, 1);
        if (b >= 0 && (lane == 63 || bn != b)) {
#pragma unroll
          for (int j = 0; j < NS; ++j) wd_h[j * js + b] += s[j];
          wc_h[b] += (unsigned long long)sc;
        }
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
        if (lane == 0) {
#pragma unroll
          for (int j = 0; j < NS; ++j) wd_h[j * js + bb] += s[j];
          wc_h[bb] += (unsigned long long)sc;
        }
        rem &= ~__ballot(mine);
      }
    }
  }
  __syncthreads();
  const long long base = (long long)blockIdx.x * nb;
  for (int i = tid; i < nb; i += nthreads) {
    double s[NS] = {0.0, 0.0, 0.0, 0.0};
    unsigned long long c = 0ull;
    for (int v = 0; v < nw; ++v) {
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] += hd[j * js + v * nb + i];
      c += hc[v * nb + i];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) pd[j * plane_words + base + i] = s[j];
    pc[base + i] = c;
  }
}

// The same sweep for rows of at least 64 * CELLS cells with a kz2 table that does not decrease (multipole_launch_shape: `cells`): a lane
// takes CELLS consecutive cells of the row, so that CELLS loads are in flight per lane and one scan serves 64 * CELLS cells.  The
// bins of a lane's cells form runs.  A run strictly inside the lane -- neither its first nor its last -- belongs to no other lane and
// is added to the histogram by the lane itself.  The last run (the only one, if the bins do not change) goes into the segmented scan
// keyed by its bin: a lane whose bins change starts a key larger than every key before it, so equal keys are still neighbouring lanes.
// The first run of a lane whose bins change ends the run of the lanes before it: the lane adds the scan's value of the lane before
// (if that lane's key is this bin) to its own part and adds the total to the histogram; a lane adds its scanned run itself only when
// the next lane's first bin differs.  No two lanes add to one bin in the same instruction, and every order is fixed.  Dropped cells
// carry bin -1 and zeros: -1 is never added, and a row's valid cells are one block, so the runs of valid bins stay contiguous.
// A wave without a single binned cell in a step skips the step (decided by a ballot: whole waves).
template <typename T, int CELLS>
__global__ __launch_bounds__(256) void multipole_sweep_cells_kernel(const cplx<T>* __restrict__ S, MultipoleParams gm, const double* __restrict__ e2_dev,
                                                                    unsigned nrows, unsigned long long* __restrict__ pc, double* __restrict__ pd,
                                                                    long long plane_words) {
  extern __shared__ double multipole_lds[];
  const int nb = gm.p.nbins;
  const int nthreads = blockDim.x * blockDim.y, tid = threadIdx.y * blockDim.x + threadIdx.x;
  const int nw = nthreads >> 6, wave = tid >> 6, lane = tid & 63;
  double* e2 = multipole_lds;                               // [nb + 1]
  double* hd = e2 + (nb + 1);                               // [NS][nw][nb]
  unsigned long long* hc = reinterpret_cast<unsigned long long*>(hd + NS * nw * nb);   // [nw][nb]
  for (int i = tid; i <= nb; i += nthreads) e2[i] = e2_dev[i];
  for (int i = tid; i < NS * nw * nb; i += nthreads) hd[i] = 0.0;
  for (int i = tid; i < nw * nb; i += nthreads) hc[i] = 0ull;
  __syncthreads();
  const int nzh = gm.p.nz / 2 + 1;
  double* wd_h = hd + wave * nb;
  const int js = nw * nb;
  unsigned long long* wc_h = hc + wave * nb;
  for (unsigned long long r0 = (unsigned long long)blockIdx.x * blockDim.y; r0 < nrows; r0 += (unsigned long long)gridDim.x * blockDim.y) {
    const unsigned long long rr = r0 + threadIdx.y;
    const bool row_ok = rr < nrows;
    const unsigned row = row_ok ? (unsigned)rr : 0u, ix = row / (unsigned)gm.p.ny, iy = row - ix * (unsigned)gm.p.ny;
    for (int iz0 = 0; iz0 < nzh; iz0 += blockDim.x * CELLS) {
      const int izb = iz0 + threadIdx.x * CELLS;
      cplx<T> v[CELLS];
#pragma unroll
      for (int c = 0; c < CELLS; ++c)
        if (row_ok && izb + c < nzh) v[c] = power_load<T>(gm.p, S, (int)ix, (int)iy, izb + c);
      // the lane's runs: `head` is the first run once the bins have changed (hb = -2: they have not), `cur` the run being summed
      int b0 = -1, hb = -2, hw = 0, cb = -1, cw = 0;
      double hs[NS] = {0.0, 0.0, 0.0, 0.0}, cs[NS] = {0.0, 0.0, 0.0, 0.0};
      bool any = false;
#pragma unroll
      for (int c = 0; c < CELLS; ++c) {
        int b = -1, w = 0;
        double d[NS] = {0.0, 0.0, 0.0, 0.0};
        if (row_ok && izb + c < nzh) {
          double m[3];
          b = multipole_cell<T>(gm, e2, v[c], (int)ix, (int)iy, izb + c, w, d[0], m);
          d[1] = m[0]; d[2] = m[1]; d[3] = m[2];
        }
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
#pragma unroll
            for (int j = 0; j < NS; ++j) wd_h[j * js + cb] += cs[j];
            wc_h[cb] += (unsigned long long)cw;
          }
          cb = b; cw = w;
#pragma unroll
          for (int j = 0; j < NS; ++j) cs[j] = d[j];
        }
      }
      if (__ballot(any) == 0ull) continue;
      // segmented inclusive scan of the lanes' last runs, keyed by their bins
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int bo = __shfl_up(cb, off);
        double t[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) t[j] = __shfl_up(cs[j], off);
        const int tc = __shfl_up(cw, off);
        if (lane >= off && bo == cb) {
#pragma unroll
          for (int j = 0; j < NS; ++j) cs[j] += t[j];
          cw += tc;
        }
      }
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
#pragma unroll
        for (int j = 0; j < NS; ++j) wd_h[j * js + hb] += hs[j];
        wc_h[hb] += (unsigned long long)hw;
      }
      if (cb >= 0 && (lane == 63 || nb0 != cb)) {
#pragma unroll
        for (int j = 0; j < NS; ++j) wd_h[j * js + cb] += cs[j];
        wc_h[cb] += (unsigned long long)cw;
      }
    }
  }
  __syncthreads();
  const long long base = (long long)blockIdx.x * nb;
  for (int i = tid; i < nb; i += nthreads) {
    double s[NS] = {0.0, 0.0, 0.0, 0.0};
    unsigned long long c = 0ull;
    for (int v = 0; v < nw; ++v) {
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] += hd[j * js + v * nb + i];
      c += hc[v * nb + i];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) pd[j * plane_words + base + i] = s[j];
    pc[base + i] = c;
  }
}

// out = the nwg rows of the partial planes summed in row order: 16 bins x 16 chunks of rows per workgroup, the chunks of a bin combined
// in chunk order.  oc: [count nbins], od: [sum_k nbins][m0 nbins][m2 nbins][m4 nbins]
__global__ __launch_bounds__(256) void multipole_reduce_kernel(const unsigned long long* __restrict__ pc, const double* __restrict__ pd,
                                                               long long plane_words, int nwg, int nb, unsigned long long* __restrict__ oc,
                                                               double* __restrict__ od) {
  __shared__ double rd[NS][16][17];
  __shared__ unsigned long long rc[16][17];
  const int bl = threadIdx.x & 15, ch = threadIdx.x >> 4, b = blockIdx.x * 16 + bl;
  const int per = (nwg + 15) / 16, lo = ch * per, hi = lo + per < nwg ? lo + per : nwg;
  double s[NS] = {0.0, 0.0, 0.0, 0.0};
  unsigned long long c = 0ull;
  if (b < nb) {
#pragma unroll 4
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

}  // namespace

MultipoleLaunch multipole_launch_shape(int nx, int ny, int nz, int nbins) {
  MultipoleLaunch L;
  // a wave's histogram takes 40 bytes per bin (four float64 sums and the count) behind the nbins + 1 edges: four waves per workgroup up
  // to 384 bins, two up to 736, one above stay inside 64 KB of LDS (at 1024 bins: 57 KB)
  const int nthreads = nbins <= 384 ? 256 : (nbins <= 736 ? 128 : 64);
  const int nzh = nz / 2 + 1;
  // rows of at least 256 cells: four cells per lane (multipole_sweep_cells_kernel, if kz2 is sorted), threads along kz for a quarter of the row
  L.cells = nzh >= 256 ? 4 : 1;
  const int span = (nzh + L.cells - 1) / L.cells;
  int tx = 1;
  while (tx < nthreads && tx < span) tx <<= 1;
  L.tx = tx;
  L.ty = nthreads / tx;
  const long long nrows = (long long)nx * ny, nblk = (nrows + L.ty - 1) / L.ty;
  const long long cap = nbins <= 128 ? 2048 : 1024;        // workgroups: rows of the partial planes (<= 2^20 words per plane)
  L.grid = (unsigned)(nblk < cap ? (nblk < 1 ? 1 : nblk) : cap);
  L.lds = (size_t)((nbins + 1) + MULTIPOLE_PLANES * (nthreads / 64) * nbins) * 8;
  return L;
}

hipError_t launch_multipoles(int f64, const void* S, const MultipoleParams& gm, const double* e2_dev, unsigned long long* partials,
                             long long plane_words, unsigned long long* out, hipStream_t s) {
  const PowerParams& gp = gm.p;
  const long long nrows = (long long)gp.nx * gp.ny;
  if (nrows <= 0 || nrows > 0x7fffffffLL || gp.nbins < 1 || gp.nbins > 1024 || (gp.nz & 1) || gm.los < 0 || gm.los > 2) return hipErrorInvalidValue;
  const MultipoleLaunch L = multipole_launch_shape(gp.nx, gp.ny, gp.nz, gp.nbins);
  if ((long long)L.grid * gp.nbins > plane_words || L.lds > 65536) return hipErrorInvalidValue;
  unsigned long long* pc = partials;
  double* pd = reinterpret_cast<double*>(partials + plane_words);
  const dim3 grid(L.grid), block(L.tx, L.ty);
  if (L.cells == 4 && gp.kz_sorted && L.tx >= 64) {
    if (f64) hipLaunchKernelGGL((multipole_sweep_cells_kernel<double, 4>), grid, block, L.lds, s, (const cplx<double>*)S, gm, e2_dev, (unsigned)nrows, pc, pd, plane_words);
    else hipLaunchKernelGGL((multipole_sweep_cells_kernel<float, 4>), grid, block, L.lds, s, (const cplx<float>*)S, gm, e2_dev, (unsigned)nrows, pc, pd, plane_words);
  } else {
    if (f64) hipLaunchKernelGGL(multipole_sweep_kernel<double>, grid, block, L.lds, s, (const cplx<double>*)S, gm, e2_dev, (unsigned)nrows, pc, pd, plane_words);
    else hipLaunchKernelGGL(multipole_sweep_kernel<float>, grid, block, L.lds, s, (const cplx<float>*)S, gm, e2_dev, (unsigned)nrows, pc, pd, plane_words);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(multipole_reduce_kernel, dim3((unsigned)((gp.nbins + 15) / 16)), dim3(256), 0, s, pc, pd, plane_words, (int)L.grid, gp.nbins, out,
                     reinterpret_cast<double*>(out + gp.nbins));
  return hipGetLastError();
}

}  // namespace rf
