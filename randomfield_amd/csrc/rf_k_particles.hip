// particles (rf_core.h cic_axis ... cic_delta): the resident displacement buffer's fma sweep and the two cloud-in-cell operations over the
// displaced lattice particles.  One walk per launch form (cic_global_kernel, cic_tiled_kernel) and one launcher (cic_launch) serve both; an
// operation is a policy struct that says what happens before the particles of a brick, with one particle's eight cells, with a dropped
// particle, and after the brick:
//   PaintOp   the scatter into an unsigned 64-bit accumulator grid.  Integer atomics only -- vector (global) and LDS ones: integer
//             addition is associative, so the accumulator holds the same bits for every launch shape, either form and every run.  No
//             floating-point atomics.
//   GatherOp  the scatter's adjoint (rf_core.h cic_gather_value): the field gathered at the particles, no atomics but the drop counter's.
// The operation also names the assignment scheme -- its per-axis type (Op::Axis) and how a particle is located (Op::locate): cloud in
// cell for these two, the triangular-shaped cloud (27 cells, rf_core.h tsc_*) for TscPaintOp / TscGatherOp, which inherit the rest.
// The two paint operations also come shifted by half a cell on every axis (HALF; rf_core.h cic_axis_half): the second grid of an
// interlaced paint, whose two spectra rf_k_misc.hip's interlace_kernel combines.
#include "rf_kernels.h"
#include "rf_launch.h"

namespace rf {
namespace {

typedef unsigned long long u64;

// Form 2's geometry: a workgroup owns a brick of BX x BY x BZ lattice cells (BZ = 64: a wave takes one z row of the brick, so its lanes
// hit consecutive LDS and memory addresses) and a tile image of brick + halo H in LDS, CIC_TILE_CELLS elements of the operation's type.
constexpr int CIC_BX = 8, CIC_BY = 8, CIC_BZ = 64, CIC_H = 2, CIC_NT = 512;
constexpr int CIC_TILE_CELLS = (CIC_BX + 2 * CIC_H) * (CIC_BY + 2 * CIC_H) * (CIC_BZ + 2 * CIC_H);      // 12 x 12 x 68 = 9792 cells, 78336 bytes of 8
static_assert(2 * CIC_TILE_CELLS * 8 <= 163840, "two workgroups per compute unit");
// (one array for both operations, in the paint's element type: the paint indexes it as it stands -- through a pointer its LDS
// addresses cost an instruction more per access -- and the gather views it as T)
extern __shared__ __attribute__((aligned(16))) u64 cic_lds[];

// The paint.  Global: eight no-return 64-bit integer atomics straight into A (a wave's adds to one of the eight corners are 512
// contiguous bytes wherever the displacement varies slowly).  Tiled: LDS 64-bit integer atomics into the cleared tile; particles whose
// eight cells do not all fall inside the tile add straight into A as the global form does.  The tile is flushed with one global atomic
// per non-zero tile cell, indices wrapped periodically there: neighbouring bricks' halos overlap, bricks at the grid's edge are partial,
// and on a grid smaller than the tile several tile cells alias one cell of A -- the atomic flush covers all three.
// HALF: the particle at u + 1/2 on every axis (rf_core.h cic_axis_half), the second grid of an interlaced paint.  A template parameter of
// the operation, so the unshifted instantiations are the code they were; everything past locate() is shared.
template <typename T, bool HALF = false>
struct PaintOp {
  typedef u64 Cell;
  typedef CicAxis Axis;
  u64* __restrict__ A;
  static __device__ bool locate(T sx, T sy, T sz, const CicGrid& g, int ix, int iy, int iz, Axis& x, Axis& y, Axis& z) {
    if (HALF) return cic_particle_half<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
    return cic_particle<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
  }
  __device__ void prologue(const CicTile&, const CicGrid&, int tid) const {
    for (int s = tid; s < CIC_TILE_CELLS; s += CIC_NT) cic_lds[s] = 0ull;
  }
  __device__ void particle(long long, const CicAxis& x, const CicAxis& y, const CicAxis& z, const CicGrid& g) const {
    cic_scatter_global(x, y, z, g.ny, g.nz, [&](long long cell, uint64_t w) { atomicAdd(A + cell, (u64)w); });
  }
  __device__ void particle(long long, const CicAxis& x, const CicAxis& y, const CicAxis& z, int lx, int ly, int lz, const CicTile& t,
                           const CicGrid& g) const {
    cic_scatter_tiled(x, y, z, lx, ly, lz, t, g.ny, g.nz, [&](int slot, uint64_t w) { atomicAdd(&cic_lds[slot], (u64)w); },
                      [&](long long cell, uint64_t w) { atomicAdd(A + cell, (u64)w); });
  }
  __device__ void dropped(long long) const {}
  __device__ void epilogue(const CicTile& t, const CicGrid& g, int tid) const {
    __syncthreads();                                   // (every wave's adds are in the tile)
    __builtin_assume(tid >= 0 && tid < CIC_NT);        // (cic_tile_cell divides s: 16-bit arithmetic, as with threadIdx.x in its place)
    for (int s = tid; s < CIC_TILE_CELLS; s += CIC_NT) {
      const u64 v = cic_lds[s];
      if (v) atomicAdd(A + cic_tile_cell(t, s, g.nx, g.ny, g.nz), v);
    }
  }
};

// The gather: the field W at the particles into G, every particle writing its own element of G (read first unless `first`), coalesced.
// Global: eight plain loads of W through the caches.  Tiled: the workgroup stages W at the tile's cells (cic_tile_cell: periodic wrap,
// partial bricks and grids smaller than the tile are all in that map) into LDS with coalesced loads; a particle whose eight cells lie
// inside the tile reads them there (a wave's lanes on consecutive addresses), any other reads W as the global form does.
template <typename T>
struct GatherOp {
  typedef T Cell;
  typedef CicAxis Axis;
  const T* __restrict__ W;
  T* __restrict__ G;
  double coeff;
  int first;
  static __device__ T* tile() { return reinterpret_cast<T*>(cic_lds); }
  static __device__ bool locate(T sx, T sy, T sz, const CicGrid& g, int ix, int iy, int iz, Axis& x, Axis& y, Axis& z) {
    return cic_particle<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
  }
  __device__ void prologue(const CicTile& t, const CicGrid& g, int tid) const {
    __builtin_assume(tid >= 0 && tid < CIC_NT);        // (as in PaintOp::epilogue)
    for (int s = tid; s < CIC_TILE_CELLS; s += CIC_NT) tile()[s] = W[cic_tile_cell(t, s, g.nx, g.ny, g.nz)];
  }
  __device__ void out(long long i, double v) const { G[i] = cic_gather_out<T>(first != 0, coeff, v, first ? (T)0 : G[i]); }
  __device__ void particle(long long i, const CicAxis& x, const CicAxis& y, const CicAxis& z, const CicGrid& g) const {
    out(i, cic_gather_global(x, y, z, g.ny, g.nz, [&](long long cell) { return (double)W[cell]; }));
  }
  __device__ void particle(long long i, const CicAxis& x, const CicAxis& y, const CicAxis& z, int lx, int ly, int lz, const CicTile& t,
                           const CicGrid& g) const {
    out(i, cic_gather_tiled(x, y, z, lx, ly, lz, t, g.ny, g.nz, [&](int slot) { return (double)tile()[slot]; },
                            [&](long long cell) { return (double)W[cell]; }));
  }
  __device__ void dropped(long long i) const { if (first) G[i] = (T)0; }
  __device__ void epilogue(const CicTile&, const CicGrid&, int) const {}
};

// The same two operations with the triangular-shaped cloud (rf_core.h tsc_axis ... tsc_gather_tiled): 27 cells per particle where cloud
// in cell has eight.  The tile, its clearing, staging and flush are the cloud-in-cell operations' own; only what happens with one
// particle differs.
template <typename T, bool HALF = false>
struct TscPaintOp : PaintOp<T> {
  typedef TscAxis Axis;
  static __device__ bool locate(T sx, T sy, T sz, const CicGrid& g, int ix, int iy, int iz, Axis& x, Axis& y, Axis& z) {
    if (HALF) return tsc_particle_half<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
    return tsc_particle<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
  }
  __device__ void particle(long long, const Axis& x, const Axis& y, const Axis& z, const CicGrid& g) const {
    u64* A = this->A;
    tsc_scatter_global(x, y, z, g.ny, g.nz, [&](long long cell, uint64_t w) { atomicAdd(A + cell, (u64)w); });
  }
  __device__ void particle(long long, const Axis& x, const Axis& y, const Axis& z, int lx, int ly, int lz, const CicTile& t, const CicGrid& g) const {
    u64* A = this->A;
    tsc_scatter_tiled(x, y, z, lx, ly, lz, t, g.ny, g.nz, [&](int slot, uint64_t w) { atomicAdd(&cic_lds[slot], (u64)w); },
                      [&](long long cell, uint64_t w) { atomicAdd(A + cell, (u64)w); });
  }
};
template <typename T>
struct TscGatherOp : GatherOp<T> {
  typedef TscAxis Axis;
  static __device__ bool locate(T sx, T sy, T sz, const CicGrid& g, int ix, int iy, int iz, Axis& x, Axis& y, Axis& z) {
    return tsc_particle<T>(sx, sy, sz, g.inv_h, ix, iy, iz, g.nx, g.ny, g.nz, x, y, z);
  }
  __device__ void particle(long long i, const Axis& x, const Axis& y, const Axis& z, const CicGrid& g) const {
    const T* W = this->W;
    this->out(i, tsc_gather_global(x, y, z, g.ny, g.nz, [&](long long cell) { return (double)W[cell]; }));
  }
  __device__ void particle(long long i, const Axis& x, const Axis& y, const Axis& z, int lx, int ly, int lz, const CicTile& t, const CicGrid& g) const {
    const T* W = this->W;
    this->out(i, tsc_gather_tiled(x, y, z, lx, ly, lz, t, g.ny, g.nz, [&](int slot) { return (double)GatherOp<T>::tile()[slot]; },
                                  [&](long long cell) { return (double)W[cell]; }));
  }
};

// the wave's dropped particles -> one integer atomic (nothing when the wave dropped none)
__device__ __forceinline__ void cic_count_dropped(int mine, u64* dropped) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(dropped, (u64)mine);
}

// Form 1, global: one lane per particle, lanes along z, the operation's eight cells straight in memory.  blockDim.x is a multiple of 64.
template <typename T, class Op>
__global__ __launch_bounds__(256) void cic_global_kernel(const T* __restrict__ Qx, const T* __restrict__ Qy, const T* __restrict__ Qz, Op op,
                                                         u64* __restrict__ dropped, CicGrid g, long long n) {
  int ndrop = 0;
  const long long step = (long long)gridDim.x * blockDim.x;
  // (every lane of a wave runs the same number of steps: the shuffles below see whole waves)
  for (long long i0 = (long long)blockIdx.x * blockDim.x; i0 < n; i0 += step) {
    const long long i = i0 + threadIdx.x;
    if (i >= n) continue;
    int ix, iy, iz;
    cic_lattice(i, g.ny, g.nz, ix, iy, iz);
    typename Op::Axis x, y, z;
    if (!Op::locate(Qx[i], Qy[i], Qz[i], g, ix, iy, iz, x, y, z)) { ++ndrop; op.dropped(i); continue; }
    op.particle(i, x, y, z, g);
  }
  cic_count_dropped(ndrop, dropped);
}

// Form 2, tiled: the workgroup of brick blockIdx.x; a wave takes one z row of the brick at a time (the trip count is the same for
// every lane of a wave: the shuffles of cic_count_dropped see whole waves)
template <typename T, class Op>
__global__ __launch_bounds__(CIC_NT) void cic_tiled_kernel(const T* __restrict__ Qx, const T* __restrict__ Qy, const T* __restrict__ Qz, Op op,
                                                           u64* __restrict__ dropped, CicGrid g, int nby, int nbz) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CicTile t = cic_brick_tile(blockIdx.x, nby, nbz, CIC_BX, CIC_BY, CIC_BZ, CIC_H);
  op.prologue(t, g, tid);
  __syncthreads();
  int ndrop = 0;
  const int iz = t.z0 + lane;
  for (int row = wave; row < CIC_BX * CIC_BY; row += CIC_NT / 64) {
    const int lx = row / CIC_BY, ly = row - lx * CIC_BY, ix = t.x0 + lx, iy = t.y0 + ly;
    if (ix >= g.nx || iy >= g.ny || iz >= g.nz) continue;
    const long long i = ((long long)ix * g.ny + iy) * g.nz + iz;
    typename Op::Axis x, y, z;
    if (!Op::locate(Qx[i], Qy[i], Qz[i], g, ix, iy, iz, x, y, z)) { ++ndrop; op.dropped(i); continue; }
    op.particle(i, x, y, z, lx, ly, lane, t, g);
  }
  op.epilogue(t, g, tid);
  cic_count_dropped(ndrop, dropped);
}

// W = (double)A 2^-48 - 1 rounded once to T (rf_core.h cic_delta)
template <typename T>
__global__ __launch_bounds__(256) void cic_convert_kernel(const u64* __restrict__ A, T* __restrict__ W, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) W[i] = cic_delta<T>(A[i]);
}

// Q = coeff W (first) or fma(coeff, W, Q), shaped like lpt2_accumulate_kernel: VEC elements (16 bytes) per lane and array, grid-strided
// (every axis of a plan is even, so the arrays are whole numbers of 16 bytes)
template <typename T, int VEC, bool FIRST>
__global__ __launch_bounds__(256) void particles_accumulate_kernel(const T* __restrict__ W, T* __restrict__ Q, T coeff, long long nvec) {
  typedef T vt __attribute__((ext_vector_type(VEC)));
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const vt w = __builtin_nontemporal_load(reinterpret_cast<const vt*>(W) + i);
    vt q;
    if (!FIRST) q = __builtin_nontemporal_load(reinterpret_cast<const vt*>(Q) + i);
#pragma unroll
    for (int e = 0; e < VEC; ++e) q[e] = particles_axpy<T>(FIRST, coeff, w[e], FIRST ? (T)0 : q[e]);
    __builtin_nontemporal_store(q, reinterpret_cast<vt*>(Q) + i);
  }
}

inline unsigned sweep_grid(long long n, int block) {
  long long g = (n + block - 1) / block;
  if (g > 256 * 16) g = 256 * 16;          // (the grid-stride loops beyond it: tests/test_gpu_at_scale.py)
  return (unsigned)(g < 1 ? 1 : g);
}

template <typename T, int VEC>
hipError_t particles_accumulate_t(const T* W, T* Q, double coeff, int first, long long n, hipStream_t s) {
  if (n <= 0 || n % VEC || (uintptr_t)W % 16 || (uintptr_t)Q % 16) return hipErrorInvalidValue;
  const long long nvec = n / VEC;
  const dim3 grid(sweep_grid(nvec, 256)), block(256);
  const T c = (T)coeff;
  if (first) hipLaunchKernelGGL((particles_accumulate_kernel<T, VEC, true>), grid, block, 0, s, W, Q, c, nvec);
  else hipLaunchKernelGGL((particles_accumulate_kernel<T, VEC, false>), grid, block, 0, s, W, Q, c, nvec);
  return hipGetLastError();
}

// both forms of one operation over the particles displaced by Q[3][nx][ny][nz]
template <typename T, class Op>
hipError_t cic_launch(int form, const T* Q, const Op& op, u64* dropped, int nx, int ny, int nz, const double* inv_h, hipStream_t s) {
  const long long n = (long long)nx * ny * nz;
  const CicGrid g = {nx, ny, nz, {inv_h[0], inv_h[1], inv_h[2]}};
  const T *Qx = Q, *Qy = Q + n, *Qz = Q + 2 * n;
  if (form == 1) {
    hipLaunchKernelGGL((cic_global_kernel<T, Op>), dim3(sweep_grid(n, 256)), dim3(256), 0, s, Qx, Qy, Qz, op, dropped, g, n);
    return hipGetLastError();
  }
  const long long nbx = (nx + CIC_BX - 1) / CIC_BX, nby = (ny + CIC_BY - 1) / CIC_BY, nbz = (nz + CIC_BZ - 1) / CIC_BZ;
  const long long nb = nbx * nby * nbz;
  if (nb > 0x7fffffffLL) return hipErrorInvalidValue;
  static LdsAttrLatch latch;
  const int lds = CIC_TILE_CELLS * (int)sizeof(typename Op::Cell);      // 78 336 bytes, the float32 gather 39 168: two workgroups per compute unit
  if (hipError_t e = latch.ensure(reinterpret_cast<const void*>(&cic_tiled_kernel<T, Op>), lds)) return e;
  hipLaunchKernelGGL((cic_tiled_kernel<T, Op>), dim3((unsigned)nb), dim3(CIC_NT), lds, s, Qx, Qy, Qz, op, dropped, g, (int)nby, (int)nbz);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_cic_gather(int f64, int scheme, int form, const void* Q, const void* W, void* G_slot, double coeff, int first, unsigned long long* dropped,
                             int nx, int ny, int nz, const double* inv_h, hipStream_t s) {
  if (nx < 1 || ny < 1 || nz < 1 || (form != 1 && form != 2)) return hipErrorInvalidValue;
  if (scheme == 3) {
    return f64 ? cic_launch(form, (const double*)Q, TscGatherOp<double>{{(const double*)W, (double*)G_slot, coeff, first}}, dropped, nx, ny, nz, inv_h, s)
               : cic_launch(form, (const float*)Q, TscGatherOp<float>{{(const float*)W, (float*)G_slot, coeff, first}}, dropped, nx, ny, nz, inv_h, s);
  }
  if (scheme != 2) return hipErrorInvalidValue;
  return f64 ? cic_launch(form, (const double*)Q, GatherOp<double>{(const double*)W, (double*)G_slot, coeff, first}, dropped, nx, ny, nz, inv_h, s)
             : cic_launch(form, (const float*)Q, GatherOp<float>{(const float*)W, (float*)G_slot, coeff, first}, dropped, nx, ny, nz, inv_h, s);
}

hipError_t launch_particles_accumulate(int f64, const void* W, void* Q, double coeff, int first, long long n, hipStream_t s) {
  return f64 ? particles_accumulate_t<double, 2>((const double*)W, (double*)Q, coeff, first, n, s)
             : particles_accumulate_t<float, 4>((const float*)W, (float*)Q, coeff, first, n, s);
}

namespace {
template <bool HALF>
hipError_t cic_paint_t(int f64, int scheme, int form, const void* Q, u64* A, u64* dropped, int nx, int ny, int nz, const double* inv_h, hipStream_t s) {
  if (scheme == 3) {
    return f64 ? cic_launch(form, (const double*)Q, TscPaintOp<double, HALF>{{A}}, dropped, nx, ny, nz, inv_h, s)
               : cic_launch(form, (const float*)Q, TscPaintOp<float, HALF>{{A}}, dropped, nx, ny, nz, inv_h, s);
  }
  if (scheme != 2) return hipErrorInvalidValue;
  return f64 ? cic_launch(form, (const double*)Q, PaintOp<double, HALF>{A}, dropped, nx, ny, nz, inv_h, s)
             : cic_launch(form, (const float*)Q, PaintOp<float, HALF>{A}, dropped, nx, ny, nz, inv_h, s);
}
}  // namespace

hipError_t launch_cic_paint(int f64, int scheme, int form, int half_cell, const void* Q, unsigned long long* A, unsigned long long* dropped, int nx, int ny,
                            int nz, const double* inv_h, hipStream_t s) {
  if (nx < 1 || ny < 1 || nz < 1 || (form != 1 && form != 2) || (half_cell != 0 && half_cell != 1)) return hipErrorInvalidValue;
  return half_cell ? cic_paint_t<true>(f64, scheme, form, Q, A, dropped, nx, ny, nz, inv_h, s)
                   : cic_paint_t<false>(f64, scheme, form, Q, A, dropped, nx, ny, nz, inv_h, s);
}

void cic_paint_geometry(int* brick3, int* halo) {
  brick3[0] = CIC_BX; brick3[1] = CIC_BY; brick3[2] = CIC_BZ;
  *halo = CIC_H;
}

hipError_t launch_cic_convert(int f64, const unsigned long long* A, void* W, long long n, hipStream_t s) {
  if (n <= 0) return hipErrorInvalidValue;
  if (f64) hipLaunchKernelGGL(cic_convert_kernel<double>, dim3(sweep_grid(n, 256)), dim3(256), 0, s, A, (double*)W, n);
  else hipLaunchKernelGGL(cic_convert_kernel<float>, dim3(sweep_grid(n, 256)), dim3(256), 0, s, A, (float*)W, n);
  return hipGetLastError();
}

}  // namespace rf
