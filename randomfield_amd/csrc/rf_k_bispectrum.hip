// the kernels of rf_measure_bispectrum (rf_core.h shell_cell / bispectrum_add): the shell filter that restricts the half spectrum to one
// k shell, and the triple-product reduction over the nbins shell fields.  No floating-point atomics anywhere: the same plan, data,
// edges and triples give the same bits on every call.
#include "rf_kernels.h"
#include "rf_launch.h"

namespace rf {
namespace {

// M = shell_cell(K) over the API-layout half spectrum [nx][ny][nz/2 + 1]: rows (ix, iy) as derivative_kernel walks them, blockDim.x
// threads along kz, blockDim.y rows per workgroup, a grid-stride loop over the rows.  The squared edges (at most 33) go to LDS.
template <typename T>
__global__ __launch_bounds__(256) void shell_filter_kernel(const cplx<T>* __restrict__ K, cplx<T>* __restrict__ M, ShellParams g,
                                                           const double* __restrict__ e2_dev, int shell, unsigned nrows) {
  __shared__ double e2[BISPECTRUM_MAX_BINS + 1];
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  if (tid <= g.p.nbins) e2[tid] = e2_dev[tid];
  __syncthreads();
  const int nzh = g.p.nz / 2 + 1;
  for (unsigned long long r0 = (unsigned long long)blockIdx.x * blockDim.y; r0 < nrows; r0 += (unsigned long long)gridDim.x * blockDim.y) {
    const unsigned long long rr = r0 + threadIdx.y;
    if (rr >= nrows) continue;
    const unsigned row = (unsigned)rr, ix = row / (unsigned)g.p.ny, iy = row - ix * (unsigned)g.p.ny;
    const cplx<T>* Kr = K + (long long)row * nzh;
    cplx<T>* Mr = M + (long long)row * nzh;
    for (int iz = threadIdx.x; iz < nzh; iz += blockDim.x) Mr[iz] = shell_cell<T>(g, e2, shell, Kr[iz], (int)ix, (int)iy, iz);
  }
}

// s(t) = sum over cells x of D_b1(x) D_b2(x) D_b3(x) for every triple t at once.  F: the nbins dense shell fields, field b at F + b ncells.
// A workgroup stages a chunk of `chunk` cells of all nbins fields into LDS (tile[b][c], one pass over the fields whatever the number of
// triples), then every thread walks the chunk for the triples it owns: per cell three LDS reads and bispectrum_add, the sums kept in
// registers across the grid-stride loop over chunks.  One partial per (workgroup, cell group, triple); bispectrum_reduce_kernel adds
// them in row order.
// Threads: 256 = ncg cell groups x nslots triple slots (nslots 64, 128 or 256: whole waves).  Thread (cg, slot) owns the triples
// tile0 + slot + j nslots, j < TPT, and the cell pairs 2 (cg + i ncg) of the chunk: with few triples (<= 128) the groups share the
// cells instead of idling.  More than 256 TPT triples: the next tile of triples is blockIdx.y, which streams the fields again -- once
// per 256 TPT >= 256 triples, never per triple.
// LDS banks: the lanes of a wave read the SAME cell pair of DIFFERENT fields (equal fields broadcast).  A lane's address is
// b pitch + c elements, pitch = chunk + 2 with chunk a multiple of 64: in units of the 8-byte (float32 pair) or 16-byte (float64 pair)
// access that is b (pitch / 2) + c / 2 with pitch / 2 odd, so the fields 0 .. 31 of a float32 plan fall into 32 different 8-byte bank
// pairs (ds_read_b64: conflict-free), and those of a float64 plan into 16 different 16-byte groups per 16 fields (ds_read_b128 serves
// 16 lanes per cycle: b and b + 16 share a group, at worst two-way).
// Cells past the end of the fields are staged as zeros: they add an exact 0.
template <typename T, int TPT>
__global__ __launch_bounds__(256) void bispectrum_sum_kernel(const T* __restrict__ F, long long ncells, int nbins, int chunk, long long nchunks,
                                                             const unsigned* __restrict__ triples, int ntriples, int nslots,
                                                             double* __restrict__ partials) {
  typedef T pair_t __attribute__((ext_vector_type(2)));
  extern __shared__ double bispectrum_lds[];
  T* tile = reinterpret_cast<T*>(bispectrum_lds);
  const int pitch = chunk + 2, tid = threadIdx.x;
  const int ncg = 256 / nslots, slot = tid % nslots, cg = tid / nslots;
  const int tile0 = blockIdx.y * nslots * TPT;
  int o1[TPT], o2[TPT], o3[TPT];
  double s[TPT];
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int t = tile0 + slot + j * nslots;
    const unsigned w = t < ntriples ? triples[t] : 0u;      // (a slot without a triple walks (0, 0, 0) and writes nothing)
    o1[j] = (int)(w & 255u) * pitch; o2[j] = (int)((w >> 8) & 255u) * pitch; o3[j] = (int)((w >> 16) & 255u) * pitch;
    s[j] = 0.0;
  }
  const int npair = chunk / 2;
  for (long long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const long long c0 = ch * chunk;
    __syncthreads();                                         // (the chunk before has been read by every thread)
    for (int b = 0; b < nbins; ++b) {
      const T* Fb = F + (long long)b * ncells + c0;
      for (int q = tid; q < npair; q += 256) {
        pair_t v = {(T)0, (T)0};
        if (c0 + 2 * q < ncells) v = *reinterpret_cast<const pair_t*>(Fb + 2 * q);      // (ncells and c0 are even: a pair is inside or outside)
        *reinterpret_cast<pair_t*>(tile + b * pitch + 2 * q) = v;
      }
    }
    __syncthreads();
    for (int c = 2 * cg; c < chunk; c += 2 * ncg) {
#pragma unroll
      for (int j = 0; j < TPT; ++j) {
        const pair_t x = *reinterpret_cast<const pair_t*>(tile + o1[j] + c);
        const pair_t y = *reinterpret_cast<const pair_t*>(tile + o2[j] + c);
        const pair_t z = *reinterpret_cast<const pair_t*>(tile + o3[j] + c);
        s[j] = bispectrum_add(s[j], (double)x[0], (double)y[0], (double)z[0]);
        s[j] = bispectrum_add(s[j], (double)x[1], (double)y[1], (double)z[1]);
      }
    }
  }
  const long long prow = ((long long)blockIdx.x * ncg + cg) * ntriples;
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int t = tile0 + slot + j * nslots;
    if (t < ntriples) partials[prow + t] = s[j];
  }
}

// out[t] = the nrows partial rows of triple t summed in row order: 16 triples x 16 runs of rows per workgroup, the runs of a triple
// combined in run order (as bin_reduce_kernel)
__global__ __launch_bounds__(256) void bispectrum_reduce_kernel(const double* __restrict__ partials, int nrows, int ntriples, double* __restrict__ out) {
  __shared__ double rd[16][17];
  const int tl = threadIdx.x & 15, run = threadIdx.x >> 4, t = blockIdx.x * 16 + tl;
  const int per = (nrows + 15) / 16, lo = run * per, hi = lo + per < nrows ? lo + per : nrows;
  double s = 0.0;
  if (t < ntriples)
    for (int r = lo; r < hi; ++r) s += partials[(long long)r * ntriples + t];
  rd[run][tl] = s;
  __syncthreads();
  if (run == 0 && t < ntriples) {
    s = 0.0;
    for (int v = 0; v < 16; ++v) s += rd[v][tl];
    out[t] = s;
  }
}

}  // namespace

hipError_t launch_shell_filter(int f64, const void* K, void* M, const ShellParams& g, const double* e2_dev, int shell, int max_workgroups, hipStream_t s) {
  const long long nrows = (long long)g.p.nx * g.p.ny;
  const int nzh = g.p.nz / 2 + 1;
  if (nrows <= 0 || nrows > 0x7fffffffLL || g.p.nz < 2 || (g.p.nz & 1) || g.p.nbins < 1 || g.p.nbins > BISPECTRUM_MAX_BINS || shell < 0 || shell >= g.p.nbins ||
      !K || !M || K == M)
    return hipErrorInvalidValue;
  int tx = 1;
  while (tx < 256 && tx < nzh) tx <<= 1;
  const int ty = 256 / tx;
  const long long nblk = (nrows + ty - 1) / ty, cap = max_workgroups > 0 ? max_workgroups : 256 * 16;
  const unsigned grid = (unsigned)(nblk < cap ? nblk : cap);
  if (f64) hipLaunchKernelGGL(shell_filter_kernel<double>, dim3(grid), dim3(tx, ty), 0, s, (const cplx<double>*)K, (cplx<double>*)M, g, e2_dev, shell, (unsigned)nrows);
  else hipLaunchKernelGGL(shell_filter_kernel<float>, dim3(grid), dim3(tx, ty), 0, s, (const cplx<float>*)K, (cplx<float>*)M, g, e2_dev, shell, (unsigned)nrows);
  return hipGetLastError();
}

BispectrumLaunch bispectrum_launch_shape(int f64, long long ncells, int nbins, int ntriples, int max_workgroups) {
  BispectrumLaunch L;
  const int esize = f64 ? 8 : 4;
  // the tile [nbins][chunk + 2] inside 40 KB: four workgroups per CU (160 KB), chunk a multiple of 64 cells
  // (32 bins: 256 cells of a float32 plan, 128 of a float64 one; 8 bins: 1216 and 576)
  int chunk = ((BISPECTRUM_LDS_BYTES / (nbins * esize) - 2) / 64) * 64;
  L.chunk = chunk < 64 ? 64 : chunk;
  L.lds = (size_t)nbins * (L.chunk + 2) * esize;
  L.nchunks = (ncells + L.chunk - 1) / L.chunk;
  L.nslots = ntriples <= 64 ? 64 : (ntriples <= 128 ? 128 : 256);
  L.tpt = ntriples <= 256 ? 1 : (ntriples <= 512 ? 2 : (ntriples <= 768 ? 3 : 4));      // (564 closed triples of 16 bins: 768 slots, not 1024)
  const int tile = L.nslots * L.tpt;
  L.gy = (unsigned)((ntriples + tile - 1) / tile);
  const long long cap = max_workgroups > 0 ? max_workgroups : BISPECTRUM_MAX_WORKGROUPS;
  L.gx = (unsigned)(L.nchunks < cap ? (L.nchunks < 1 ? 1 : L.nchunks) : cap);
  L.rows = (int)L.gx * (256 / L.nslots);
  return L;
}

hipError_t launch_bispectrum_sums(int f64, const void* F, long long ncells, int nbins, const unsigned* triples_dev, int ntriples, int max_workgroups,
                                  double* partials, double* out, hipStream_t s) {
  if (ncells <= 0 || (ncells & 1) || nbins < 1 || nbins > BISPECTRUM_MAX_BINS || ntriples < 1 || ntriples > BISPECTRUM_MAX_TRIPLES || !F || !triples_dev ||
      !partials || !out || (uintptr_t)F % 16)
    return hipErrorInvalidValue;
  const BispectrumLaunch L = bispectrum_launch_shape(f64, ncells, nbins, ntriples, max_workgroups);
  if (L.lds > 65536) return hipErrorInvalidValue;
  const dim3 grid(L.gx, L.gy), block(256);
#define RF_BISPECTRUM(T, TPT) \
  hipLaunchKernelGGL((bispectrum_sum_kernel<T, TPT>), grid, block, L.lds, s, (const T*)F, ncells, nbins, L.chunk, L.nchunks, triples_dev, ntriples, L.nslots, partials)
  if (f64) {
    if (L.tpt == 1) RF_BISPECTRUM(double, 1); else if (L.tpt == 2) RF_BISPECTRUM(double, 2); else if (L.tpt == 3) RF_BISPECTRUM(double, 3); else RF_BISPECTRUM(double, 4);
  } else {
    if (L.tpt == 1) RF_BISPECTRUM(float, 1); else if (L.tpt == 2) RF_BISPECTRUM(float, 2); else if (L.tpt == 3) RF_BISPECTRUM(float, 3); else RF_BISPECTRUM(float, 4);
  }
#undef RF_BISPECTRUM
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bispectrum_reduce_kernel, dim3((unsigned)((ntriples + 15) / 16)), dim3(256), 0, s, partials, L.rows, ntriples, out);
  return hipGetLastError();
}

}  // namespace rf
