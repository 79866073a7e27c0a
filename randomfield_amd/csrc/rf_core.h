// rf_core.h -- arithmetic shared by every kernel of the MI355X random-field path.
//
// Everything here is plain C++ templates marked RF_HD so that the same code is
// (a) inlined into the HIP kernels for gfx950 and (b) compiled by g++ into the
// CPU kernel emulator (csrc/emu) that checks index math, twiddles and phase
// structure in the build container, where there is no GPU.
//
// Reference rows restated here:
//   K  powertools.py:27-61   |k| per cell            -> log10k_cell()
//   T  powertools.py:125-164 sigma(k) table lookup   -> sigma_lookup()
//   R  random.py:12-29       sigma * N(0,1)          -> gen_cell()
//   S  transform.py:141-158  Hermitian symmetrise    -> sym_role(), gen_cell()
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RF_HD __host__ __device__ __forceinline__
#define RF_DEVICE_CODE 1
#else
#define RF_HD inline
#endif

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace rf {

// ---------------------------------------------------------------- complex --
template <typename T>
struct cplx {
  T x, y;
};

template <typename T> RF_HD cplx<T> mk(T x, T y) { cplx<T> r; r.x = x; r.y = y; return r; }
template <typename T> RF_HD cplx<T> operator+(cplx<T> a, cplx<T> b) { return mk<T>(a.x + b.x, a.y + b.y); }
template <typename T> RF_HD cplx<T> operator-(cplx<T> a, cplx<T> b) { return mk<T>(a.x - b.x, a.y - b.y); }
template <typename T> RF_HD cplx<T> cmul(cplx<T> a, cplx<T> b) {
  return mk<T>(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
template <typename T> RF_HD cplx<T> cconj(cplx<T> a) { return mk<T>(a.x, -a.y); }
// multiply by +i (DIR=+1) or -i (DIR=-1)
template <int DIR, typename T> RF_HD cplx<T> mul_i(cplx<T> a) {
  return DIR > 0 ? mk<T>(-a.y, a.x) : mk<T>(a.y, -a.x);
}
// conjugate the twiddle for the forward transform: tables hold exp(+2 pi i q/N)
template <int DIR, typename T> RF_HD cplx<T> tw_dir(cplx<T> w) { return DIR > 0 ? w : mk<T>(w.x, -w.y); }

// ------------------------------------------------------- radix butterflies --
// DFT<R, DIR>::run(v): in-place R-point DFT, natural order in and out,
// kernel exp(DIR * 2 pi i n k / R).  DIR=+1 is the (unnormalised) inverse.
template <int R, int DIR> struct DFT;

template <int DIR> struct DFT<1, DIR> {
  template <typename T> RF_HD static void run(cplx<T>*) {}
};

template <int DIR> struct DFT<2, DIR> {
  template <typename T> RF_HD static void run(cplx<T>* v) {
    cplx<T> a = v[0], b = v[1];
    v[0] = a + b;
    v[1] = a - b;
  }
};

template <int DIR> struct DFT<4, DIR> {
  template <typename T> RF_HD static void run(cplx<T>* v) {
    cplx<T> t0 = v[0] + v[2], t1 = v[0] - v[2];
    cplx<T> t2 = v[1] + v[3], t3 = mul_i<DIR>(v[1] - v[3]);
    v[0] = t0 + t2;
    v[1] = t1 + t3;
    v[2] = t0 - t2;
    v[3] = t1 - t3;
  }
};

// exp(DIR * 2 pi i q / 16) for q = 0..9 (products n2*k1 of the 4x4 split)
template <int DIR, typename T> RF_HD cplx<T> w16(int q) {
  const T c1 = (T)0.92387953251128675613, s1 = (T)0.38268343236508977173, r = (T)0.70710678118654752440;
  T cx, sy;
  switch (q) {
    case 0: cx = 1; sy = 0; break;
    case 1: cx = c1; sy = s1; break;
    case 2: cx = r; sy = r; break;
    case 3: cx = s1; sy = c1; break;
    case 4: cx = 0; sy = 1; break;
    case 6: cx = -r; sy = r; break;
    default: cx = -c1; sy = -s1; break;  // q == 9
  }
  return mk<T>(cx, DIR > 0 ? sy : -sy);
}

template <int DIR> struct DFT<8, DIR> {
  // n = 2 n1 + n2, k = k1 + 4 k2
  template <typename T> RF_HD static void run(cplx<T>* v) {
    cplx<T> a[4] = {v[0], v[2], v[4], v[6]};
    cplx<T> b[4] = {v[1], v[3], v[5], v[7]};
    DFT<4, DIR>::run(a);
    DFT<4, DIR>::run(b);
    const T r = (T)0.70710678118654752440;
    // w8^k1 = exp(DIR 2 pi i k1 / 8)
    b[1] = cmul(b[1], mk<T>(r, DIR > 0 ? r : -r));
    b[2] = mul_i<DIR>(b[2]);
    b[3] = cmul(b[3], mk<T>(-r, DIR > 0 ? r : -r));
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
      v[k1] = a[k1] + b[k1];
      v[k1 + 4] = a[k1] - b[k1];
    }
  }
};

template <int DIR> struct DFT<16, DIR> {
  // n = 4 n1 + n2, k = k1 + 4 k2
  template <typename T> RF_HD static void run(cplx<T>* v) {
    cplx<T> a[4][4];
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) {
#pragma unroll
      for (int n1 = 0; n1 < 4; ++n1) a[n2][n1] = v[4 * n1 + n2];
      DFT<4, DIR>::run(a[n2]);  // a[n2][k1]
    }
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
      cplx<T> c[4];
      c[0] = a[0][k1];
#pragma unroll
      for (int n2 = 1; n2 < 4; ++n2) c[n2] = (k1 == 0) ? a[n2][k1] : cmul(a[n2][k1], w16<DIR, T>(n2 * k1));
      DFT<4, DIR>::run(c);  // c[k2]
#pragma unroll
      for (int k2 = 0; k2 < 4; ++k2) v[k1 + 4 * k2] = c[k2];
    }
  }
};

// ----------------------------------------------------------- Stockham maps --
// Pass with radix R on sub-transforms of length Ns (Ns = product of earlier
// radices): butterfly j in [0, N/R) reads in[j + m*N/R], multiplies by
// exp(DIR 2 pi i m (j % Ns) / (Ns R)), does an R-point DFT, writes
// out[(j / Ns) * Ns * R + (j % Ns) + m * Ns].  Natural order after the last pass.
RF_HD int stockham_out_base(int j, int Ns, int R) { return (j / Ns) * Ns * R + (j % Ns); }
// index into a length-N table of exp(2 pi i q / N)
RF_HD int stockham_tw_index(int j, int m, int Ns, int R, int N) { return m * (j % Ns) * (N / (Ns * R)); }

// -------------------------------------------------------------------- RNG --
struct PhiloxOut { uint32_t w[4]; };

RF_HD uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// Philox4x32-R (Salmon, Moraes, Dror, Shaw 2011).  counter = (ctr_lo, ctr_hi) as
// two 64-bit words, key = 64-bit seed.
// A workgroup-uniform 64-bit value pinned to scalar registers: keeps the compiler from re-associating
// (lane part) + (uniform part) sums back into per-lane 64-bit multiplies.
RF_HD uint64_t pin_uniform(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
  return ((uint64_t)hi << 32) | lo;
#else
  return x;
#endif
}

RF_HD long long pin_uniform_ll(long long x) { return (long long)pin_uniform((uint64_t)x); }

RF_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);      // one v_bitop3_b32 instead of two v_xor_b32
#else
  return a ^ b ^ c;
#endif
}

// Rounds of the NATIVE stream: Philox4x32-7 is the smallest round count the authors found Crush-resistant (SC'11, table 2: it
// passes BigCrush); the library default of 10 is a safety margin.  The generation pass is VALU-bound and a Philox round costs
// two v_mad_u64_u32 + two v_bitop3 per lane-load: 7 instead of 10 rounds is -6 % of its instructions (measured -1.3 % of a
// 1024^3 realisation).  The test-side restatement of the stream uses the same count; both are pinned by Random123's
// published known-answer vectors for 7 and 10 rounds (tests/test_oracle_golden.py).
constexpr int PHILOX_ROUNDS = 7;          // the native stream's definition (CHANGES.md): Philox4x32-7
template <int ROUNDS = PHILOX_ROUNDS>
RF_HD PhiloxOut philox4x32(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) {
  uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32);
  uint32_t c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    // one 32x32->64 product each (v_mad_u64_u32), not separate mul_lo / mul_hi
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
    const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0;
    const uint32_t h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
    uint32_t n0 = xor3(h1, c1, k0), n2 = xor3(h0, c3, k1);
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  PhiloxOut o; o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}
RF_HD PhiloxOut philox_native(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) { return philox4x32<PHILOX_ROUNDS>(ctr_lo, ctr_hi, key); }

// Box-Muller from two 32-bit words: u = (w + 0.5) / 2^32 in (0, 1).
template <typename T> struct BoxMuller;
template <> struct BoxMuller<double> {
  RF_HD static void run(uint32_t wa, uint32_t wb, double& g0, double& g1) {
    double u1 = ((double)wa + 0.5) * (1.0 / 4294967296.0);
    double u2 = ((double)wb + 0.5) * (1.0 / 4294967296.0);
    double r = sqrt(-2.0 * log(u1));
#if defined(__HIP_DEVICE_COMPILE__)
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);       // no Payne-Hanek style reduction: the argument is an exact multiple of pi
    g0 = r * cs;
    g1 = r * sn;
#else
    double a = (2.0 * M_PI) * u2;
    g0 = r * cos(a);
    g1 = r * sin(a);
#endif
  }
};
template <> struct BoxMuller<float> {
  // (g0, g1) = scale * N(0,1) pair.
  // u1 = (w + 1/2) / 2^32 formed as ONE fused multiply-add of float(w): the float keeps 24 significant bits at
  // any magnitude, so the radius resolves the tail down to u1 = 2^-33 (6.7 sigma); u1 is never 0 (it may round
  // to exactly 1, giving radius 0).  The angle uses the top 23 bits of its word: u2 = (w >> 9) / 2^23 revolutions.
  RF_HD static void run_scaled(uint32_t wa, uint32_t wb, float scale, float& g0, float& g1) {
    const float u1 = fmaf((float)wa, 1.0f / 4294967296.0f, 1.0f / 8589934592.0f);
#if defined(__HIP_DEVICE_COMPILE__)
    // raw v_log_f32 / v_sqrt_f32: u1 >= 2^-33 and -2 ln u1 in [0, 46) need no denormal fix-ups.
    // -2 ln u = (-2 ln 2) log2 u
    const float r = scale * __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
    // the float with exponent 0 and mantissa w >> 9 is 1 + u2 (one v_alignbit_b32); v_sin_f32 / v_cos_f32 take
    // their argument in revolutions and reduce it themselves
    const float rev = __uint_as_float(__builtin_amdgcn_alignbit(0x7Fu, wb, 9));
    g0 = r * __builtin_amdgcn_cosf(rev);
    g1 = r * __builtin_amdgcn_sinf(rev);
#else
    const float r = scale * sqrtf(-2.0f * logf(u1));
    const float a = (float)(2.0 * M_PI) * ((float)(wb >> 9) * (1.0f / 8388608.0f));
    g0 = r * cosf(a);
    g1 = r * sinf(a);
#endif
  }
  RF_HD static void run(uint32_t wa, uint32_t wb, float& g0, float& g1) { run_scaled(wa, wb, 1.0f, g0, g1); }
};

// ------------------------------------------------------------ generation --
enum { NOISE_PHILOX = 0, NOISE_EXTERNAL = 1 };

struct GenParams {
  int nx, ny, nz;             // real-space grid
  const double* kx2;          // [nx]      k_x(i)^2, float64, host-computed as powertools.py:27-37
  const double* ky2;          // [ny]
  const double* kz2;          // [nz/2+1]
  const double* xt;           // [nt] log10 k_i      (powertools.py:153)
  const double* st;           // [nt] sigma_i        (powertools.py:154)
  const double* sl;           // [nt-1] (st[j+1]-st[j])/(xt[j+1]-xt[j])
  const int* bin;             // [nbins] acceleration grid: lower bound of the interval index per bin
  int nt, nbins;
  double x0, inv_dx;          // bin b covers x0 + [b, b+1) / inv_dx
  int noise_mode;
  uint64_t seed;
  const uint64_t* seed_dev;   // if non-null the seed is read from device memory (graph replay)
  const double* noise;        // external mode: 2*nx*ny*(nz/2+1) float64 deviates, reference order
  // The API-layout side arrays (noise, k space, potential) of a kz-slab rank hold its planes only: rows of `zpitch`
  // slots, slot j < zpitch - 1 = plane zoff + j, the last slot = the Nyquist plane kz = nz/2 (which rank 0 packs into
  // its slot kz = 0).  One rank: zpitch = nz/2 + 1, zoff = 0 -- the reference's layout itself.
  int zpitch, zoff;
};

// slot of plane kz in a row of a side array (GenParams / FastGenParams)
template <class G> RF_HD int side_slot(const G& g, int kz) { return kz == g.nz / 2 ? g.zpitch - 1 : kz - g.zoff; }

// no-FMA arithmetic: these must round exactly like numpy's separate ufunc calls / numpy's C code built
// without FMA.  (hipcc contracts a*b+c by default and its __dmul_rn/__dadd_rn are plain operators, so the
// contraction is switched off by pragma; the host build parks the product in a volatile.)
RF_HD double mul_then_add(double a, double b, double c) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double p = a * b;
  return p + c;
#else
  volatile double p = a * b;
  return p + c;
#endif
}
RF_HD double sum_of_squares(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double p = a * a, q = b * b;
  return p + q;
#else
  volatile double p = a * a, q = b * b;
  return p + q;
#endif
}

// The edge rule of row T.  The reference zeroes sigma outside the table (interp1d fill_value = 0, powertools.py:155-157) and asks
// the table to cover every grid mode (powertools.py:147-150).  A table that ends exactly on the grid's own k_min or k_max
// passes that check with the fundamental or corner modes ON its edge, and the last bit of log10|k| -- numpy's loop, libm, OCML
// and v_log_f32 all round differently -- would decide whether those modes exist.  So: a non-DC cell whose log10|k| lies outside
// the table by no more than RF_EDGE_TOL takes the edge row's sigma; anything further outside stays 0.
// RF_EDGE_TOL is twice what the float32 chains can lose on x = log10|k| for |x| < 4 (k > 1e-4):
//   exact chain (sigma_cell<float>): two roundings of |k|^2, 2 * 2^-24 relative = 0.5 log10(e) * 1.2e-7 = 2.6e-8 dex; log10f of
//     |k|^2 (|.| < 8: one ulp is 4.8e-7) times 0.5 (exact) = 2.4e-7 dex per ulp of the implementation, 1 - 2 ulp:     <= 5e-7 dex
//   fast chain (fast_sigma): u = log2|k|^2 * u_scale + u_off locates x - x0 = u dx; the roundings of u_scale, u_off and of the
//     product cost 2^-24 |x| each, v_log_f32 (1 ulp) 2^-23 |x|, the sum 2^-24 (x - x0): 6e-8 (5 |x| + span) = 1e-6 dex at |x| = 2.6
//     over 3 decades (the 3e-5 of a bin >= 4e-3 dex wide that the float32 u resolves is the smallest term)              ~ 1e-6 dex
// (float64 plans round x to 1e-16; the same rule holds there).  build_fast_records (rf_host.h) evaluates the fast chain's bound
// for the table at hand and declines when it exceeds RF_EDGE_TOL.
constexpr double RF_EDGE_TOL = 2e-6;

// Row T: piecewise-linear sigma(log10 k), 0 outside the table (powertools.py:155-157,163) but for the edge rule above.
RF_HD double sigma_lookup(const GenParams& g, double x) {
  const int n = g.nt;
  if (!(x >= g.xt[0] - RF_EDGE_TOL && x <= g.xt[n - 1] + RF_EDGE_TOL)) return 0.0;  // also -inf (DC cell) and NaN
  if (x >= g.xt[n - 1]) return g.st[n - 1];
  if (x < g.xt[0]) return g.st[0];
  int b = (int)((x - g.x0) * g.inv_dx);
  b = b < 0 ? 0 : (b >= g.nbins ? g.nbins - 1 : b);
  int j = g.bin[b];
  while (j > 0 && g.xt[j] > x) --j;
  while (j < n - 2 && g.xt[j + 1] <= x) ++j;
  return mul_then_add(g.sl[j], x - g.xt[j], g.st[j]);
}

// Row K + T: sigma of cell (ix, iy, iz), rounded to the array's real type.
template <typename T> RF_HD T sigma_cell(const GenParams& g, int ix, int iy, int iz);
template <> RF_HD float sigma_cell<float>(const GenParams& g, int ix, int iy, int iz) {
  float t = (float)(g.kx2[ix] + g.ky2[iy]);          // powertools.py:50
  t = (float)((double)t + g.kz2[iz]);                 // powertools.py:52
  t = log10f(t) * 0.5f;                               // powertools.py:56,60  (-inf at DC)
  return (float)sigma_lookup(g, (double)t);           // powertools.py:163
}
template <> RF_HD double sigma_cell<double>(const GenParams& g, int ix, int iy, int iz) {
  double t = g.kx2[ix] + g.ky2[iy];
  t = t + g.kz2[iz];
  t = log10(t) * 0.5;
  return sigma_lookup(g, t);
}

// Native noise index of API cell (ix, iy, iz): cells with iz < nz/2 are numbered
// in the device-internal order [ix][iy][nz/2]; the Nyquist plane follows.
RF_HD uint64_t native_noise_index(const GenParams& g, int ix, int iy, int iz) {
  const uint64_t nzc = (uint64_t)(g.nz / 2);
  const uint64_t col = (uint64_t)ix * (uint64_t)g.ny + (uint64_t)iy;
  return iz < g.nz / 2 ? col * nzc + (uint64_t)iz : (uint64_t)g.nx * (uint64_t)g.ny * nzc + col;
}

// Row R deviates (g_re, g_im) of the cell that OWNS the draw.
template <typename T>
RF_HD void noise_of_cell(const GenParams& g, uint64_t seed, int ix, int iy, int iz, double& gre, double& gim) {
  if (g.noise_mode == NOISE_EXTERNAL) {
    const uint64_t c = ((uint64_t)ix * (uint64_t)g.ny + (uint64_t)iy) * (uint64_t)g.zpitch + (uint64_t)side_slot(g, iz);
    gre = g.noise[2 * c];
    gim = g.noise[2 * c + 1];
  } else {
    const uint64_t ci = native_noise_index(g, ix, iy, iz);
    PhiloxOut o = philox_native(ci >> 1, 0, seed);
    T a, b;
    if (ci & 1) BoxMuller<T>::run(o.w[2], o.w[3], a, b);
    else        BoxMuller<T>::run(o.w[0], o.w[1], a, b);
    gre = (double)a;
    gim = (double)b;
  }
}

// Row S roles inside a kz in {0, nz/2} plane (transform.py:141-158).
enum { RF_SRC = 0, RF_DEST = 1, RF_SELF = 2 };
RF_HD int sym_role(int nx, int ny, int ix, int iy) {
  const bool xe = (ix == 0) || (ix == nx / 2);
  const bool ye = (iy == 0) || (iy == ny / 2);
  if (xe && ye) return RF_SELF;
  if (iy > ny / 2) return RF_DEST;
  if (ye && ix > nx / 2) return RF_DEST;
  return RF_SRC;
}

// Rows K,T,R,S for one API cell (ix, iy, iz), iz in [0, nz/2].
template <typename T>
RF_HD cplx<T> gen_cell(const GenParams& g, uint64_t seed, int ix, int iy, int iz) {
  int sx = ix, sy = iy, role = RF_SRC;
  if (iz == 0 || iz == g.nz / 2) {
    role = sym_role(g.nx, g.ny, ix, iy);
    if (role == RF_DEST) {  // take conj of the draw at (-ix, -iy)
      sx = (g.nx - ix) % g.nx;
      sy = (g.ny - iy) % g.ny;
    }
  }
  const T s = sigma_cell<T>(g, sx, sy, iz);
  double gre, gim;
  noise_of_cell<T>(g, seed, sx, sy, iz, gre, gim);
  T re = (T)((double)s * gre);       // random.py:28: product in float64, rounded once
  T im = (T)((double)s * gim);
  if (role == RF_DEST) im = -im;
  if (role == RF_SELF) im = (T)0;    // transform.py:154-156
  if (ix == 0 && iy == 0 && iz == 0) re = (T)0;  // transform.py:158
  return mk<T>(re, im);
}

// Device-internal packed cell: kz in [0, nz/2); slot kz = 0 carries
// A(kz=0) + i * A(kz=nz/2)  (both planes are 2-D Hermitian, so after the x and
// y inverse passes they are real and occupy re / im of one complex plane).
template <typename T>
RF_HD cplx<T> gen_packed(const GenParams& g, uint64_t seed, int ix, int iy, int kz) {
  cplx<T> a = gen_cell<T>(g, seed, ix, iy, kz);
  if (kz == 0) {
    cplx<T> n = gen_cell<T>(g, seed, ix, iy, g.nz / 2);
    a = mk<T>(a.x - n.y, a.y + n.x);
  }
  return a;
}

// ----------------------------------------------- gradient of the potential --
// One component of the vector field of the saved potential: psi_a(k) = i k_a phi(k), phi = delta(k) / k^2, so that div psi = -delta
// (displacements, and with a per-plane factor velocities).  k_a = dk * m with m the signed mode number of the cell along the axis;
// m = 0 at the axis' own Nyquist index (i k is not Hermitian there) and at index 0, so those planes -- the DC cell among them -- are
// exactly zero.  `divide`: the source holds delta(k), not delta(k) / k^2, and the factor takes the 1 / k^2 (sum of the plan's tables
// in float64).  The factor is formed in float64 and rounded ONCE to the array's real type; the products are the second rounding.
struct GradParams {
  int nx, ny, nz;             // real-space grid; cells of the half spectrum [nx][ny][nz/2+1]
  int axis;                   // 0, 1, 2: x, y, z
  int divide;                 // the source holds delta(k): divide by k^2
  double sdk;                 // scale * dk, dk = 2 pi / (n_axis spacing)
  const double* kx2;          // the k^2 tables of GenParams (read in divide mode only)
  const double* ky2;
  const double* kz2;
  long long pitch;            // cells per row (ix, iy) of the SOURCE array (nz/2 + 1, or the potential's padded pitch)
};
// signed mode number of index i of an axis of n points (half: the z axis of the half spectrum, i in [0, n/2])
RF_HD int grad_mode(int i, int n, bool half) {
  if (2 * i == n) return 0;
  return (half || 2 * i < n) ? i : i - n;
}
template <typename T>
RF_HD cplx<T> grad_cell(const GradParams& g, cplx<T> v, int ix, int iy, int iz) {
  const int m = g.axis == 0 ? grad_mode(ix, g.nx, false) : (g.axis == 1 ? grad_mode(iy, g.ny, false) : grad_mode(iz, g.nz, true));
  if (m == 0) return mk<T>((T)0, (T)0);            // (also keeps the 0 / 0 of the DC cell out of divide mode)
  double fd = g.sdk * (double)m;
  if (g.divide) fd = fd / ((g.kx2[ix] + g.ky2[iy]) + g.kz2[iz]);
  const T f = (T)fd;
  return mk<T>(-(f * v.y), f * v.x);
}

// ------------------------------------------- second-order (2LPT) source ------
// One component of the Hessian of the potential: H_ab(k) = D_a D_b phi(k) = -scale (dk_a m_a)(dk_b m_b) phi(k), D_a the spectral
// derivative of grad_cell (m = 0 at index 0 and at the axis' own Nyquist index -- on the diagonal a = b too, so that H_ab is exactly
// "the gradient applied twice").  Cells with m_a m_b = 0 are exact zeros, the DC cell among them.  The real factor is formed in
// float64, takes the 1 / k^2 in divide mode, and is rounded ONCE to the array's real type; the two products are the second rounding
// (the budget of grad_cell).  pitch, divide and the tables: as GradParams.
struct HessParams {
  int nx, ny, nz;
  int a, b;                   // 0 <= a <= b <= 2
  int divide;
  double sdk2;                // -scale * dk_a * dk_b
  const double* kx2;
  const double* ky2;
  const double* kz2;
  long long pitch;
};
RF_HD int hess_axis_mode(const HessParams& g, int axis, int ix, int iy, int iz) {
  return axis == 0 ? grad_mode(ix, g.nx, false) : (axis == 1 ? grad_mode(iy, g.ny, false) : grad_mode(iz, g.nz, true));
}
template <typename T>
RF_HD cplx<T> hess_cell(const HessParams& g, cplx<T> v, int ix, int iy, int iz) {
  const int ma = hess_axis_mode(g, g.a, ix, iy, iz), mb = g.b == g.a ? ma : hess_axis_mode(g, g.b, ix, iy, iz);
  if (ma == 0 || mb == 0) return mk<T>((T)0, (T)0);
  double fd = g.sdk2 * ((double)ma * (double)mb);
  if (g.divide) fd = fd / ((g.kx2[ix] + g.ky2[iy]) + g.kz2[iz]);
  const T f = (T)fd;
  return mk<T>(f * v.x, f * v.y);
}

// Both cell functions under one name, chosen by the parameter struct, for the code that is written once for the two (the elementwise
// kernel, the x pass of rf_generic.h, their launchers and the emulator) ...
template <typename T> RF_HD cplx<T> deriv_cell(const GradParams& g, cplx<T> v, int ix, int iy, int iz) { return grad_cell<T>(g, v, ix, iy, iz); }
template <typename T> RF_HD cplx<T> deriv_cell(const HessParams& g, cplx<T> v, int ix, int iy, int iz) { return hess_cell<T>(g, v, ix, iy, iz); }
// ... and what every launch checks first: the axes name a component, and a row of the source holds at least the nz/2 + 1 cells read
RF_HD bool deriv_valid(const GradParams& g) { return g.axis >= 0 && g.axis <= 2 && g.pitch >= g.nz / 2 + 1; }
RF_HD bool deriv_valid(const HessParams& g) { return g.a >= 0 && g.a <= g.b && g.b <= 2 && g.pitch >= g.nz / 2 + 1; }

// The real-space sweep that turns the six components into S = sum_{a<b} (H_aa H_bb - H_ab^2), one step per component h in the fixed
// order xx, yy, zz, xy, xz, yz; t, s: the accumulators.  Explicit fma: host and device round the same number of times.
//   FIRST  t = h                       DIAG2  s = t h; t = t + h            DIAG3  s = fma(t, h, s)
//   OFF    s = fma(-h, h, s)           LAST   h = fma(-h, h, s)  (the source lands where the component was)
enum { LPT2_FIRST = 0, LPT2_DIAG2 = 1, LPT2_DIAG3 = 2, LPT2_OFF = 3, LPT2_LAST = 4 };
RF_HD float lpt2_fma(float a, float b, float c) { return fmaf(a, b, c); }
RF_HD double lpt2_fma(double a, double b, double c) { return fma(a, b, c); }
template <typename T, int STEP>
RF_HD void lpt2_step(T& h, T& t, T& s) {
  if (STEP == LPT2_FIRST) t = h;
  else if (STEP == LPT2_DIAG2) { s = t * h; t = t + h; }
  else if (STEP == LPT2_DIAG3) s = lpt2_fma(t, h, s);
  else if (STEP == LPT2_OFF) s = lpt2_fma(-h, h, s);
  else h = lpt2_fma(-h, h, s);
}

// --------------------------------------------------- binned power spectrum --
// The estimator of rf_measure_power: cell (ix, iy, iz) of the half spectrum [nx][ny][nz/2+1] of unnormalised forward-transform values
// carries k^2 = (kx2[ix] + ky2[iy]) + kz2[iz] (float64, the sum order of grad_cell) and the weight w = 1 on the planes iz = 0 and
// iz = nz/2, 2 elsewhere (the half spectrum stands for the full one).  It belongs to bin b iff e2[b] <= k^2 < e2[b+1], e2 the caller's
// edges squared once in float64 by the host: no sqrt in the decision, so np.searchsorted(edges * edges, k2, 'right') - 1 agrees
// exactly.  The DC cell and cells outside all bins are dropped.  A bin sums w (integer), w sqrt(k^2) and w (re^2 + im^2), the values
// widened to float64 first.
struct PowerParams {
  int nx, ny, nz;
  int nbins;
  int kz_sorted;              // kz2 does not decrease with iz (checked by the host): consecutive cells of a row have non-decreasing bins
  int packed;                 // the source is the packed array [nx][ny][nz/2] the tiled forward passes leave (power_load), not the API layout
  const double* kx2;
  const double* ky2;
  const double* kz2;
};
// the bin of k2 among the nbins + 1 squared edges e2, or -1
RF_HD int power_bin(const double* e2, int nbins, double k2) {
  int lo = 0, hi = nbins + 1;                   // first index with e2[index] > k2
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e2[mid] <= k2) lo = mid + 1; else hi = mid;
  }
  return (lo >= 1 && lo <= nbins) ? lo - 1 : -1;
}
// returns the bin of the cell (-1: dropped) and its three contributions
template <typename T>
RF_HD int power_cell(const PowerParams& g, const double* e2, cplx<T> v, int ix, int iy, int iz, int& w, double& wk, double& wp) {
  w = 0; wk = 0.0; wp = 0.0;
  if (ix == 0 && iy == 0 && iz == 0) return -1;
  const double k2 = (g.kx2[ix] + g.ky2[iy]) + g.kz2[iz];
  const int b = power_bin(e2, g.nbins, k2);
  if (b < 0) return -1;
  w = (iz == 0 || 2 * iz == g.nz) ? 1 : 2;
  const double re = (double)v.x, im = (double)v.y;
  wk = (double)w * sqrt(k2);
  wp = (double)w * (re * re + im * im);
  return b;
}
// cell (ix, iy, iz) of the half spectrum: from the API layout (rows of nz/2 + 1 cells), or from the packed array [nx][ny][nz/2] whose
// slot kz = 0 holds C = A0 + i A_nyq -- untangled with unpack_kspace_kernel's formula and rounded to T as that kernel rounds
template <typename T>
RF_HD cplx<T> power_load(const PowerParams& g, const cplx<T>* S, int ix, int iy, int iz) {
  const int nzc = g.nz / 2;
  const long long col = (long long)ix * g.ny + iy;
  if (!g.packed) return S[col * (nzc + 1) + iz];
  if (iz > 0 && iz < nzc) return S[col * nzc + iz];
  const cplx<T> a = S[col * nzc];
  const long long mcol = (long long)((g.nx - ix) % g.nx) * g.ny + (g.ny - iy) % g.ny;
  const cplx<T> b = S[mcol * nzc];
  if (iz == 0) return mk<T>((T)0.5 * (a.x + b.x), (T)0.5 * (a.y - b.y));
  return mk<T>((T)0.5 * (a.y + b.y), (T)0.5 * (b.x - a.x));
}

// ------------------------------------------ binned power spectrum multipoles --
// The estimator of rf_measure_multipoles: the cell, its k^2, bin and weight are power_cell's (same sum order, same power_bin, the DC cell
// and cells outside all bins dropped).  mu^2 = k_los^2 / k^2 with k_los^2 the entry of the line-of-sight axis' own table (kx2[ix],
// ky2[iy] or kz2[iz] for los = 0, 1, 2): one float64 division (a non-DC cell whose tables sum to 0 -- not a k grid -- takes mu^2 = 0).
// Window compensation c = (cx[ix] cy[iy]) cz[iz], float64 tables of nx, ny, nz/2 + 1 entries, a null table = all ones.
// e = c (re^2 + im^2), values widened to float64 first.  A bin sums w, w sqrt(k^2), w e, w (e mu^2) and w ((e mu^2) mu^2): moments of
// mu^2, every term non-negative; the Legendre combinations are the host's.  With null tables w, wk and m[0] are power_cell's w, wk, wp.
struct MultipoleParams {
  PowerParams p;
  int los;                    // 0, 1, 2: the axis mu is measured against
  const double* cx;
  const double* cy;
  const double* cz;
};
template <typename T>
RF_HD int multipole_cell(const MultipoleParams& g, const double* e2, cplx<T> v, int ix, int iy, int iz, int& w, double& wk, double (&m)[3]) {
  w = 0; wk = 0.0; m[0] = 0.0; m[1] = 0.0; m[2] = 0.0;
  if (ix == 0 && iy == 0 && iz == 0) return -1;
  const double ax = g.p.kx2[ix], ay = g.p.ky2[iy], az = g.p.kz2[iz];
  const double k2 = (ax + ay) + az;
  const int b = power_bin(e2, g.p.nbins, k2);
  if (b < 0) return -1;
  w = (iz == 0 || 2 * iz == g.p.nz) ? 1 : 2;
  const double re = (double)v.x, im = (double)v.y;
  wk = (double)w * sqrt(k2);
  double e = re * re + im * im;
  if (g.cx || g.cy || g.cz) e = (((g.cx ? g.cx[ix] : 1.0) * (g.cy ? g.cy[iy] : 1.0)) * (g.cz ? g.cz[iz] : 1.0)) * e;
  const double klos2 = g.los == 0 ? ax : (g.los == 1 ? ay : az);
  const double mu2 = k2 > 0.0 ? klos2 / k2 : 0.0;
  const double e2m = e * mu2, e4m = e2m * mu2;
  m[0] = (double)w * e;
  m[1] = (double)w * e2m;
  m[2] = (double)w * e4m;
  return b;
}

// Both estimators under one name, chosen by the parameter struct, for the code that is written once for the two (the kernels and the
// launcher of rf_k_power.hip, measure_bins of rf_capi.hip and the emulator): the number of float64 sums a bin carries beside its count,
// the cell's contributions as one array (sum 0 is sum_k in both), and the geometry both structs hold.
template <typename P> struct BinSums;
template <> struct BinSums<PowerParams> { enum { N = 2 }; };         // sum_k, sum_p
template <> struct BinSums<MultipoleParams> { enum { N = 4 }; };     // sum_k, m0, m2, m4
RF_HD const PowerParams& bin_geom(const PowerParams& g) { return g; }
RF_HD const PowerParams& bin_geom(const MultipoleParams& g) { return g.p; }
RF_HD PowerParams& bin_geom(PowerParams& g) { return g; }
RF_HD PowerParams& bin_geom(MultipoleParams& g) { return g.p; }
template <typename T>
RF_HD int bin_cell(const PowerParams& g, const double* e2, cplx<T> v, int ix, int iy, int iz, int& w, double (&d)[2]) {
  return power_cell<T>(g, e2, v, ix, iy, iz, w, d[0], d[1]);
}
template <typename T>
RF_HD int bin_cell(const MultipoleParams& g, const double* e2, cplx<T> v, int ix, int iy, int iz, int& w, double (&d)[4]) {
  double m[3];
  const int b = multipole_cell<T>(g, e2, v, ix, iy, iz, w, d[0], m);
  d[1] = m[0]; d[2] = m[1]; d[3] = m[2];
  return b;
}

// ------------------------------------------------------- binned bispectrum --
// The FFT estimator of rf_measure_bispectrum (Scoccimarro 2015; Sefusatti et al. 2016).  Shell b holds the cells power_cell puts into
// bin b -- the same k^2, the same power_bin on the same squared edges, the DC cell in no shell -- and the shell field D_b is the inverse
// transform of the half spectrum restricted to it.  The restricted cell:
//   M = keep ? (T)(amp K) : 0     amp = (ax[ix] ay[iy]) az[iz] in float64 (null table = ones), rounded once to T per component;
//                                 with all three tables null the kept cell is K itself, bit for bit
//   M = keep ? 1 : 0              the unit run (delta = 1 inside the shells: the triangle count)
enum { BISPECTRUM_MAX_BINS = 32, BISPECTRUM_MAX_TRIPLES = 8192 };
struct ShellParams {
  PowerParams p;
  int unit;
  const double* ax;
  const double* ay;
  const double* az;
};
template <typename T>
RF_HD cplx<T> shell_cell(const ShellParams& g, const double* e2, int shell, cplx<T> v, int ix, int iy, int iz) {
  if (ix == 0 && iy == 0 && iz == 0) return mk<T>((T)0, (T)0);
  const double k2 = (g.p.kx2[ix] + g.p.ky2[iy]) + g.p.kz2[iz];
  if (power_bin(e2, g.p.nbins, k2) != shell) return mk<T>((T)0, (T)0);
  if (g.unit) return mk<T>((T)1, (T)0);
  if (!(g.ax || g.ay || g.az)) return v;
  const double amp = ((g.ax ? g.ax[ix] : 1.0) * (g.ay ? g.ay[iy] : 1.0)) * (g.az ? g.az[iz] : 1.0);
  return mk<T>((T)(amp * (double)v.x), (T)(amp * (double)v.y));
}
// One term of s(b1, b2, b3) = sum over x of D_b1 D_b2 D_b3 added to a running sum: the values widened to float64, (a b) c with both
// products and the sum rounded on their own (never contracted: pragma / volatile as mul_then_add)
RF_HD double bispectrum_add(double s, double a, double b, double c) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double ab = a * b;
  const double t = ab * c;
  return s + t;
#else
  volatile double ab = a * b;
  volatile double t = ab * c;
  return s + t;
#endif
}
// a triple (b1, b2, b3), 0 <= b < 32, as the reduction's kernels and the emulator carry it: one word
RF_HD unsigned bispectrum_pack(int b1, int b2, int b3) { return (unsigned)b1 | ((unsigned)b2 << 8) | ((unsigned)b3 << 16); }

// ------------------------------------------- particles: cloud-in-cell paint --
// One particle of unit mass per lattice cell q = (ix, iy, iz), displaced by s_a(q) (length units); inv_h[a] = 1 / (grid spacing).
// Per axis, all in float64:
//   u  = (double)s * inv_h       ONE correctly rounded product, never contracted with what follows (pragma / volatile as mul_then_add)
//   c  = floor(u),  t = (uint32) floor((u - c) * 65536) in [0, 65535]   (u - c and the scaling are exact IEEE operations that numpy
//        repeats bit for bit; for -2^-54 <= u < 0 alone u - c rounds to 1 and t = 65536: all the weight on j1, the particle's own cell)
//   j0 = (i + c) mod n, formed in float64 BEFORE any conversion to integer: m = fmod(c, n) (exact, |m| < n), r = i + m (exact),
//        r += n if r < 0, r -= n if r >= n -- any finite u gives an index in [0, n);   j1 = (j0 + 1) mod n
//   w0 = 65536 - t on j0,  w1 = t on j1
// A particle adds the eight products w_x w_y w_z (exact in 64 bits; they sum to exactly 2^48) to an unsigned 64-bit accumulator grid
// A[nx][ny][nz].  Integer addition is associative: A is the same for every launch shape, kernel form, thread count and run.  A particle
// with a non-finite u on any axis (a non-finite displacement, or a product beyond the float64 range) adds nothing and is counted.
// LIMIT: fewer than 2^64 / 2^48 = 65536 particles' worth of mass may land in one cell (no detection; Gaussian initial conditions are
// orders of magnitude below it).  The field is delta = (double)A * 2^-48 - 1, rounded once to the array's real type.
struct CicAxis {
  double c;                   // floor(u): the whole-cell part of the displacement
  int j0, j1;                 // wrapped target indices
  uint32_t w0, w1;            // their integer weights, w0 + w1 = 65536
};
RF_HD bool cic_axis(double s, double inv_h, int i, int n, CicAxis& o) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double u = s * inv_h;
#else
  volatile double uv = s * inv_h;
  const double u = uv;
#endif
  if (!(fabs(u) <= 1.7976931348623157e308)) return false;      // NaN, +-inf
  const double c = floor(u);
  const double f = u - c;                                      // in [0, 1]
  const uint32_t t = (uint32_t)floor(f * 65536.0);
  const double dn = (double)n;
  const double m = fabs(c) < dn ? c : fmod(c, dn);             // (fmod(c, n) == c for |c| < n)
  double r = (double)i + m;
  if (r < 0.0) r += dn;
  if (r >= dn) r -= dn;
  o.c = c;
  o.j0 = (int)r;
  o.j1 = o.j0 + 1 == n ? 0 : o.j0 + 1;
  o.w0 = 65536u - t;
  o.w1 = t;
  return true;
}
// the three axes of one particle; false: dropped
template <typename T>
RF_HD bool cic_particle(T sx, T sy, T sz, const double* inv_h, int ix, int iy, int iz, int nx, int ny, int nz, CicAxis& x, CicAxis& y, CicAxis& z) {
  const bool okx = cic_axis((double)sx, inv_h[0], ix, nx, x), oky = cic_axis((double)sy, inv_h[1], iy, ny, y), okz = cic_axis((double)sz, inv_h[2], iz, nz, z);
  return okx && oky && okz;
}
RF_HD uint64_t cic_weight(const CicAxis& x, const CicAxis& y, const CicAxis& z, int k) {
  return (uint64_t)((k & 4) ? x.w1 : x.w0) * (uint64_t)((k & 2) ? y.w1 : y.w0) * (uint64_t)((k & 1) ? z.w1 : z.w0);
}
// the grid and its spacing as the particle kernels and the emulator's walks carry them
struct CicGrid {
  int nx, ny, nz;
  double inv_h[3];
};
// the lattice cell of particle i
RF_HD void cic_lattice(long long i, int ny, int nz, int& ix, int& iy, int& iz) {
  const long long row = i / nz;
  iz = (int)(i - row * nz); ix = (int)(row / ny); iy = (int)(row - (long long)ix * ny);
}
// the eight cells of one particle straight in memory: f(k, cell index), k = 4 cx + 2 cy + cz with c = 0 for j0 / w0 and c = 1 for j1 / w1
template <class F>
RF_HD void cic_corners_global(const CicAxis& x, const CicAxis& y, const CicAxis& z, int ny, int nz, F&& f) {
#pragma unroll
  for (int k = 0; k < 8; ++k) f(k, ((long long)((k & 4) ? x.j1 : x.j0) * ny + ((k & 2) ? y.j1 : y.j0)) * nz + ((k & 1) ? z.j1 : z.j0));
}
// the eight adds of one particle straight into A: add(cell index, weight); zero weights add nothing and are skipped
template <class Add>
RF_HD void cic_scatter_global(const CicAxis& x, const CicAxis& y, const CicAxis& z, int ny, int nz, Add&& add) {
  cic_corners_global(x, y, z, ny, nz, [&](int k, long long cell) {
    const uint64_t w = cic_weight(x, y, z, k);
    if (w) add(cell, w);
  });
}
// The tiled form: a workgroup owns the brick of lattice cells [x0, x0 + bx) x [y0, y0 + by) x [z0, z0 + bz) and a tile image of
// brick + halo h on every side, tile[tx][ty][tz] with t = b + 2 h, tile slot 0 standing for cell x0 - h (UNWRAPPED: periodic wrapping
// happens when the tile is flushed, cic_tile_cell).  A particle whose eight cells all fall inside the tile adds there; any other adds
// straight into A as cic_scatter_global does.  The test is against the WHOLE tile (cic_tile_slot: -h <= l + c <= b + h - 2 for the local
// index l), not a window around the particle: every particle with -h <= u < h stays, and one inside the brick may move much further.
struct CicTile {
  int bx, by, bz, h;
  int x0, y0, z0;
  RF_HD int tx() const { return bx + 2 * h; }
  RF_HD int ty() const { return by + 2 * h; }
  RF_HD int tz() const { return bz + 2 * h; }
  RF_HD int cells() const { return tx() * ty() * tz(); }
};
// tile slot of j0 along one axis for the particle at local index li (slot + 1 is then inside too), or -1
RF_HD int cic_tile_slot(const CicAxis& a, int li, int b, int h) {
  const double lo = (double)li + a.c;                          // (compared in float64: c may be far outside the int range)
  return (lo >= (double)-h && lo <= (double)(b + h - 2)) ? (int)lo + h : -1;
}
// the tile of brick number b, bricks numbered with z fastest among nbx x nby x nbz of them
RF_HD CicTile cic_brick_tile(unsigned b, int nby, int nbz, int bx, int by, int bz, int h) {
  const unsigned kz = b % (unsigned)nbz, kxy = b / (unsigned)nbz, ky = kxy % (unsigned)nby, kx = kxy / (unsigned)nby;
  CicTile t;
  t.bx = bx; t.by = by; t.bz = bz; t.h = h;
  t.x0 = (int)kx * bx; t.y0 = (int)ky * by; t.z0 = (int)kz * bz;
  return t;
}
template <class AddTile, class AddGlobal>
RF_HD void cic_scatter_tiled(const CicAxis& x, const CicAxis& y, const CicAxis& z, int lx, int ly, int lz, const CicTile& t, int ny, int nz,
                             AddTile&& add_tile, AddGlobal&& add_global) {
  const int sx = cic_tile_slot(x, lx, t.bx, t.h), sy = cic_tile_slot(y, ly, t.by, t.h), sz = cic_tile_slot(z, lz, t.bz, t.h);
  if (sx < 0 || sy < 0 || sz < 0) { cic_scatter_global(x, y, z, ny, nz, add_global); return; }
  const int py = t.tz(), px = t.ty() * py, base = sx * px + sy * py + sz;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t w = cic_weight(x, y, z, k);
    if (w) add_tile(base + ((k & 4) ? px : 0) + ((k & 2) ? py : 0) + (k & 1), w);
  }
}
RF_HD int cic_wrap(int v, int n) { v %= n; return v < 0 ? v + n : v; }
// the cell of A that tile slot s stands for (several slots alias one cell when the grid is smaller than the tile)
RF_HD long long cic_tile_cell(const CicTile& t, int s, int nx, int ny, int nz) {
  const int py = t.tz(), px = t.ty() * py;
  const int ax = s / px, ay = (s - ax * px) / py, az = s - ax * px - ay * py;
  return ((long long)cic_wrap(t.x0 - t.h + ax, nx) * ny + cic_wrap(t.y0 - t.h + ay, ny)) * nz + cic_wrap(t.z0 - t.h + az, nz);
}
// delta = (double)A 2^-48 - 1, rounded once to T (the scaling is exact, so a fused multiply-add gives the same bits)
template <typename T> RF_HD T cic_delta(uint64_t a) { return (T)((double)a * (1.0 / 281474976710656.0) - 1.0); }
// Q = coeff W (first) or Q + coeff W: coeff already rounded to T, one explicit fma in T (lpt2_fma), so host and device round alike
template <typename T> RF_HD T particles_axpy(bool first, T coeff, T w, T q) { return first ? coeff * w : lpt2_fma(coeff, w, q); }

// ------------------------------------------ particles: cloud-in-cell gather --
// The adjoint of the paint: the value of a real field W[nx][ny][nz] (type T) at the particle of lattice cell q, with the indices and
// weights cic_particle gives for it.  All in float64, EVERY product and EVERY sum rounded on its own (never contracted: pragma /
// volatile as mul_then_add), so numpy repeats it bit for bit; c = 0 stands for j0 / w0, c = 1 for j1 / w1:
//   v(cx,cy,cz) = (double) W[jx_cx][jy_cy][jz_cz]
//   a(cx,cy)    = (double)wz0 * v(cx,cy,0) + (double)wz1 * v(cx,cy,1)          z first: the contiguous axis
//   b(cx)       = (double)wy0 * a(cx,0)    + (double)wy1 * a(cx,1)
//   g           = ((double)wx0 * b(0) + (double)wx1 * b(1)) * 2^-48
//   out         = first ? (T)(coeff * g) : (T)((double)G[q] + coeff * g)       one rounding to T
// Zero weights are NOT skipped (0 * v is formed): a non-finite field value reaches every particle whose eight cells contain it, also
// through a weight of zero.  For integer-valued W of modest size every step is exact and g 2^48 = sum of w_x w_y w_z W over the eight
// cells: summed over the particles that is sum over the cells of A W, A the paint's grid of the same displacements -- the adjoint
// identity, exact in integers.  A particle that cic_particle drops gathers g = 0: `first` writes 0, otherwise G[q] stays; it is counted.
RF_HD double cic_lerp(uint32_t w0, uint32_t w1, double v0, double v1) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double p0 = (double)w0 * v0, p1 = (double)w1 * v1;
  return p0 + p1;
#else
  volatile double p0 = (double)w0 * v0, p1 = (double)w1 * v1;
  return p0 + p1;
#endif
}
// g of the eight values v[4 cx + 2 cy + cz]
RF_HD double cic_gather_value(const CicAxis& x, const CicAxis& y, const CicAxis& z, const double (&v)[8]) {
  const double a00 = cic_lerp(z.w0, z.w1, v[0], v[1]), a01 = cic_lerp(z.w0, z.w1, v[2], v[3]);
  const double a10 = cic_lerp(z.w0, z.w1, v[4], v[5]), a11 = cic_lerp(z.w0, z.w1, v[6], v[7]);
  const double b0 = cic_lerp(y.w0, y.w1, a00, a01), b1 = cic_lerp(y.w0, y.w1, a10, a11);
  return cic_lerp(x.w0, x.w1, b0, b1) * (1.0 / 281474976710656.0);
}
// the value G[q] takes (old: what it holds, read only when first is false)
template <typename T> RF_HD T cic_gather_out(bool first, double coeff, double g, T old) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double p = coeff * g;
#else
  volatile double pv = coeff * g;
  const double p = pv;
#endif
  return first ? (T)p : (T)((double)old + p);
}
// the eight loads of one particle straight from W: load(cell index) -> double
template <class Load>
RF_HD double cic_gather_global(const CicAxis& x, const CicAxis& y, const CicAxis& z, int ny, int nz, Load&& load) {
  double v[8];
  cic_corners_global(x, y, z, ny, nz, [&](int k, long long cell) { v[k] = load(cell); });
  return cic_gather_value(x, y, z, v);
}
// The tiled form over the scatter's tile rule (CicTile, cic_tile_slot): the tile image holds W at the cells cic_tile_cell names, and a
// particle whose eight cells all fall inside the tile reads them there, load_tile(slot) -> double; any other reads W as
// cic_gather_global does.  Same values, same operations in the same order: the same bits either way.
// (The rule is written out here as in cic_scatter_tiled, not shared: with both paths filling one v[] behind a common visitor all eight
// values are live where the paths meet, and the float64 tiled kernel takes 84 VGPRs for 82; with the three tests in a function of
// their own it takes 92.  As written each path feeds cic_gather_value by itself.)
template <class LoadTile, class LoadGlobal>
RF_HD double cic_gather_tiled(const CicAxis& x, const CicAxis& y, const CicAxis& z, int lx, int ly, int lz, const CicTile& t, int ny, int nz,
                              LoadTile&& load_tile, LoadGlobal&& load_global) {
  const int sx = cic_tile_slot(x, lx, t.bx, t.h), sy = cic_tile_slot(y, ly, t.by, t.h), sz = cic_tile_slot(z, lz, t.bz, t.h);
  if (sx < 0 || sy < 0 || sz < 0) return cic_gather_global(x, y, z, ny, nz, load_global);
  const int py = t.tz(), px = t.ty() * py, base = sx * px + sy * py + sz;
  double v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = load_tile(base + ((k & 4) ? px : 0) + ((k & 2) ? py : 0) + (k & 1));
  return cic_gather_value(x, y, z, v);
}

// ------------------------------- particles: triangular-shaped-cloud (TSC) --
// The second assignment scheme under the same walks, tile map and accumulator grid: three cells per axis where cloud in cell has two.
// Per axis everything up to t is cic_axis as it stands (u, the drop rule, c, t in [0, 65536], j0); then, all in integers:
//   up  = t >= 32768,   tau = up ? t - 32768 : t + 32768  in [0, 65535]    tau / 65536: the particle's offset from the LEFT EDGE of its
//         nearest cell  (t = 65536, the -2^-54 <= u < 0 case: up = 1, tau = 32768 -- the particle's own cell, in its middle)
//   jc  = up ? (j0 + 1) mod n : j0,   jm = (jc - 1) mod n,   jp = (jc + 1) mod n   (on an axis shorter than 3 cells two of them coincide;
//         nothing is special-cased)
//   Wm  = (65536 - tau)^2 >> 17,   Wp = tau^2 >> 17,   W0 = 65536 - Wm - Wp      (64-bit: the square reaches 2^32)
// -- (1 - s)^2 / 2, 1/2 + s - s^2 and s^2 / 2 at s = tau / 65536 in units of 2^-16.  Over all t: every weight in [0, 49153], the three
// sum to 65536 exactly, Wp - Wm = tau - 32768 exactly (the two floors drop the same fraction: the first moment is the quantised position).
// PAINT: the 27 products W_x W_y W_z (exact in 64 bits, 2^48 per particle) go to the same grid A with the same integer atomics, zero
// products skipped: cic_delta, the conversion and the 65536-particles-per-cell limit carry over.
// GATHER: float64, every product and sum rounded on its own, lerp3(w, v) = ((double)wm vm + (double)w0 v0) + (double)wp vp along z first,
// then y, then x, times 2^-48, then cic_gather_out.  Zero weights are NOT skipped.  Each z row of three values is reduced as soon as it is
// loaded: at most three a and three b values are live, never 27.
// TILE RULE: the brick, halo and tile of CicTile; with the lowest cell's offset c_lo = c + up - 1 a particle at local index l uses the tile
// on an axis when -h <= l + c_lo <= b + h - 3 (float64 comparison, as cic_tile_slot); every particle with |u| < 1.5 stays for h = 2.
// (Written beside the cloud-in-cell functions, not as one set templated on the cells per axis: those are left verbatim so that their
// kernels keep their register counts, which the comment at cic_gather_tiled shows to hang on such details.)
struct TscAxis {
  double clo;                 // c + up - 1: the whole-cell offset of the lowest of the three cells
  int j[3];                   // wrapped target indices jm, jc, jp
  uint32_t w[3];              // their integer weights Wm, W0, Wp; they sum to 65536
};
// the three weights of t in [0, 65536]
RF_HD void tsc_weights(uint32_t t, uint32_t (&w)[3]) {
  const uint32_t tau = t >= 32768u ? t - 32768u : t + 32768u;
  const uint64_t r = 65536u - tau;
  w[0] = (uint32_t)((r * r) >> 17);
  w[2] = (uint32_t)(((uint64_t)tau * tau) >> 17);
  w[1] = 65536u - w[0] - w[2];
}
// the three cells and weights from the cloud-in-cell terms (c, j0, j1, t = w1) of the same axis
RF_HD void tsc_of_cic(const CicAxis& a, int n, TscAxis& o) {
  const bool up = a.w1 >= 32768u;
  const int jc = up ? a.j1 : a.j0;
  o.clo = a.c + (up ? 0.0 : -1.0);
  o.j[0] = jc == 0 ? n - 1 : jc - 1;
  o.j[1] = jc;
  o.j[2] = jc + 1 == n ? 0 : jc + 1;
  tsc_weights(a.w1, o.w);
}
RF_HD bool tsc_axis(double s, double inv_h, int i, int n, TscAxis& o) {
  CicAxis a;
  if (!cic_axis(s, inv_h, i, n, a)) return false;
  tsc_of_cic(a, n, o);
  return true;
}
// the three axes of one particle; false: dropped
template <typename T>
RF_HD bool tsc_particle(T sx, T sy, T sz, const double* inv_h, int ix, int iy, int iz, int nx, int ny, int nz, TscAxis& x, TscAxis& y, TscAxis& z) {
  const bool okx = tsc_axis((double)sx, inv_h[0], ix, nx, x), oky = tsc_axis((double)sy, inv_h[1], iy, ny, y), okz = tsc_axis((double)sz, inv_h[2], iz, nz, z);
  return okx && oky && okz;
}
// tile slot of the lowest cell along one axis for the particle at local index li (slot + 1 and slot + 2 are then inside too), or -1
RF_HD int tsc_tile_slot(const TscAxis& a, int li, int b, int h) {
  const double lo = (double)li + a.clo;
  return (lo >= (double)-h && lo <= (double)(b + h - 3)) ? (int)lo + h : -1;
}
// the 27 cells of one particle: f(weight product, cell(cx, cy, cz)) with c = 0, 1, 2 for m, 0, p
template <class Cell, class Add>
RF_HD void tsc_scatter_cells(const TscAxis& x, const TscAxis& y, const TscAxis& z, Cell&& cell, Add&& add) {
#pragma unroll
  for (int cx = 0; cx < 3; ++cx) {
#pragma unroll
    for (int cy = 0; cy < 3; ++cy) {
      const uint64_t wxy = (uint64_t)x.w[cx] * (uint64_t)y.w[cy];
#pragma unroll
      for (int cz = 0; cz < 3; ++cz) {
        const uint64_t w = wxy * (uint64_t)z.w[cz];
        if (w) add(cell(cx, cy, cz), w);
      }
    }
  }
}
// the 27 adds of one particle straight into A: add(cell index, weight)
template <class Add>
RF_HD void tsc_scatter_global(const TscAxis& x, const TscAxis& y, const TscAxis& z, int ny, int nz, Add&& add) {
  tsc_scatter_cells(x, y, z, [&](int cx, int cy, int cz) { return ((long long)x.j[cx] * ny + y.j[cy]) * nz + z.j[cz]; }, add);
}
// the tiled form: into the tile when all 27 cells fall inside it (add_tile(slot, weight)), otherwise as tsc_scatter_global
template <class AddTile, class AddGlobal>
RF_HD void tsc_scatter_tiled(const TscAxis& x, const TscAxis& y, const TscAxis& z, int lx, int ly, int lz, const CicTile& t, int ny, int nz,
                             AddTile&& add_tile, AddGlobal&& add_global) {
  const int sx = tsc_tile_slot(x, lx, t.bx, t.h), sy = tsc_tile_slot(y, ly, t.by, t.h), sz = tsc_tile_slot(z, lz, t.bz, t.h);
  if (sx < 0 || sy < 0 || sz < 0) { tsc_scatter_global(x, y, z, ny, nz, add_global); return; }
  const int py = t.tz(), px = t.ty() * py, base = sx * px + sy * py + sz;
  tsc_scatter_cells(x, y, z, [&](int cx, int cy, int cz) { return base + cx * px + cy * py + cz; }, add_tile);
}
RF_HD double tsc_lerp3(const uint32_t (&w)[3], double vm, double v0, double vp) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double pm = (double)w[0] * vm, p0 = (double)w[1] * v0, pp = (double)w[2] * vp;
  const double s = pm + p0;
  return s + pp;
#else
  volatile double pm = (double)w[0] * vm, p0 = (double)w[1] * v0, pp = (double)w[2] * vp;
  volatile double s = pm + p0;
  return s + pp;
#endif
}
// g of the 27 values load(cx, cy, cz): a z row of three is reduced as it arrives, three rows make a b, three b make g
template <class Load>
RF_HD double tsc_gather_cells(const TscAxis& x, const TscAxis& y, const TscAxis& z, Load&& load) {
  double b[3];
#pragma unroll
  for (int cx = 0; cx < 3; ++cx) {
    double a[3];
#pragma unroll
    for (int cy = 0; cy < 3; ++cy) {
      const double vm = load(cx, cy, 0), v0 = load(cx, cy, 1), vp = load(cx, cy, 2);
      a[cy] = tsc_lerp3(z.w, vm, v0, vp);
    }
    b[cx] = tsc_lerp3(y.w, a[0], a[1], a[2]);
  }
  return tsc_lerp3(x.w, b[0], b[1], b[2]) * (1.0 / 281474976710656.0);
}
// the 27 loads of one particle straight from W: load(cell index) -> double
template <class Load>
RF_HD double tsc_gather_global(const TscAxis& x, const TscAxis& y, const TscAxis& z, int ny, int nz, Load&& load) {
  return tsc_gather_cells(x, y, z, [&](int cx, int cy, int cz) { return load(((long long)x.j[cx] * ny + y.j[cy]) * nz + z.j[cz]); });
}
// the tiled form: from the tile image when all 27 cells fall inside it (load_tile(slot) -> double), otherwise as tsc_gather_global
template <class LoadTile, class LoadGlobal>
RF_HD double tsc_gather_tiled(const TscAxis& x, const TscAxis& y, const TscAxis& z, int lx, int ly, int lz, const CicTile& t, int ny, int nz,
                              LoadTile&& load_tile, LoadGlobal&& load_global) {
  const int sx = tsc_tile_slot(x, lx, t.bx, t.h), sy = tsc_tile_slot(y, ly, t.by, t.h), sz = tsc_tile_slot(z, lz, t.bz, t.h);
  if (sx < 0 || sy < 0 || sz < 0) return tsc_gather_global(x, y, z, ny, nz, load_global);
  const int py = t.tz(), px = t.ty() * py, base = sx * px + sy * py + sz;
  return tsc_gather_cells(x, y, z, [&](int cx, int cy, int cz) { return load_tile(base + cx * px + cy * py + cz); });
}

// ------------------------------- particles: interlaced paint (half-cell shift) --
// The second grid of an interlaced paint (Sefusatti et al. 2016): the same particles on a grid shifted by half a cell on every axis, which
// is the particle at u + 1/2 on the grid as it stands.  Per axis u, the drop rule (decided on u, BEFORE the shift), c, t in [0, 65536], j0
// and j1 are cic_axis's; then, all in integers (2^-16 cell units, so the shift is exact):
//   t2 = t + 32768,  carry = t2 >= 65536,  t' = carry ? t2 - 65536 : t2  in [0, 65535]      (t = 65536 gives t' = 32768 with a carry)
//   j0' = carry ? j1 : j0,  j1' = (j0' + 1) mod n     on the WRAPPED index, never through c: for |u| >= 2^53, where c + 1 == c, it still steps
//   c'  = c + carry                                   float64; the tile-slot tests alone read it
//   w0' = 65536 - t',  w1' = t'
// The triangular-shaped cloud takes (t', j0', c') where it took (t, j0, c) (tsc_of_cic).  Counts, cic_delta, the 65536-particles-per-cell
// limit and "the same bits on every call and kernel form" carry over.  The shift is on all three axes at once; the gather has none.
RF_HD void cic_axis_half(int n, CicAxis& a) {
  const uint32_t t2 = a.w1 + 32768u;
  const bool carry = t2 >= 65536u;
  const uint32_t t = carry ? t2 - 65536u : t2;
  if (carry) { a.c += 1.0; a.j0 = a.j1; }
  a.j1 = a.j0 + 1 == n ? 0 : a.j0 + 1;
  a.w0 = 65536u - t;
  a.w1 = t;
}
template <typename T>
RF_HD bool cic_particle_half(T sx, T sy, T sz, const double* inv_h, int ix, int iy, int iz, int nx, int ny, int nz, CicAxis& x, CicAxis& y, CicAxis& z) {
  if (!cic_particle<T>(sx, sy, sz, inv_h, ix, iy, iz, nx, ny, nz, x, y, z)) return false;
  cic_axis_half(nx, x); cic_axis_half(ny, y); cic_axis_half(nz, z);
  return true;
}
template <typename T>
RF_HD bool tsc_particle_half(T sx, T sy, T sz, const double* inv_h, int ix, int iy, int iz, int nx, int ny, int nz, TscAxis& x, TscAxis& y, TscAxis& z) {
  CicAxis a, b, c;
  if (!cic_particle_half<T>(sx, sy, sz, inv_h, ix, iy, iz, nx, ny, nz, a, b, c)) return false;
  tsc_of_cic(a, nx, x); tsc_of_cic(b, ny, y); tsc_of_cic(c, nz, z);
  return true;
}

// The combine: K <- (S + p K) / 2 per cell of two half spectra, p = px[ix] py[iy] pz[iz] the phase that undoes the shift (float64 complex
// tables; powertools.interlace_phases has the default ones).  All in float64, EVERY product and EVERY sum rounded on its own (never
// contracted: pragma / volatile as mul_then_add), so numpy repeats it bit for bit with one array operation per rounding:
//   a = px py      ar = xr yr - xi yi,  ai = xr yi + xi yr          (interlace_mul; uniform along a z row)
//   p = a pz,  q = p (double)K                                      (the same form)
//   K = (T)(0.5 ((double)S + q))  per component, one rounding to T  (the halving is exact)
RF_HD void interlace_mul(double xr, double xi, double yr, double yi, double& r, double& i) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double rr = xr * yr, ii = xi * yi, ri = xr * yi, ir = xi * yr;
  r = rr - ii;
  i = ri + ir;
#else
  volatile double rr = xr * yr, ii = xi * yi, ri = xr * yi, ir = xi * yr;
  r = rr - ii;
  i = ri + ir;
#endif
}
template <typename T>
RF_HD cplx<T> interlace_cell(cplx<T> s, cplx<T> k, double ar, double ai, double zr, double zi) {
  double pr, pi, qr, qi;
  interlace_mul(ar, ai, zr, zi, pr, pi);
  interlace_mul(pr, pi, (double)k.x, (double)k.y, qr, qi);
  return mk<T>((T)(0.5 * ((double)s.x + qr)), (T)(0.5 * ((double)s.y + qi)));
}

// ------------------------------------------------- fast native generation --
// float32 plans with the native RNG do rows K,T,R,S entirely in float32: the
// values are this repo's own definition (checked against the oracle's
// restatement of the same stream to ~1e-6), so the reference's float64
// rounding chain -- which only matters for same-noise parity -- is not needed.
struct FastRec {          // 16 bytes per bin of the uniform acceleration grid in x = log10 k
  float v0;               // sigma at the bin's left edge
  float sa;               // slope of the piece at the left edge, per bin width
  float fs;               // position of the knot inside the bin in bin units (>= 1 if none)
  float ds;               // slope change at the knot, per bin width
};                        // sigma(f) = v0 + sa * f + ds * max(f - fs, 0),  f in [0, 1) the position inside the bin

// (where the float32 deviate pairs of one row of the stream live: see make_rowloc / row_pair below)
struct RowLoc {
  uint32_t off;                 // in-segment slot of the row's cell kz = 0
  uint32_t seg_n;               // (seg << 11) | nfirst,  1 <= nfirst <= nz/2 + 1 <= 1025
};
enum { ROWLOC_NBITS = 11 };

struct FastGenParams {
  int nx, ny, nz;
  float dkx, dky, dkz;    // k_axis(i) = dk_axis * signed fftfreq index (2 pi / (n spacing)): the kernels form |k|^2
                          // arithmetically, so the generation loop reads no global memory at all (on gfx950 a load
                          // would also wait for every store issued before it -- one counter for both)
  const FastRec* rec;     // global copy of the records; the kernels stage them in LDS when nbins <= FAST_LDS_BINS
  int nbins;
  float u_scale, u_off;   // bin coordinate u = log2(k^2) * u_scale + u_off
  uint64_t seed;
  const uint64_t* seed_dev;
  const double* noise;    // SRC = 1 kernels: resident float64 deviates in the reference's order (random.py:24-28),
                          // 2 per cell of the API layout [nx][ny][nz/2+1]
  int zpitch, zoff;       // row pitch and first plane of the side arrays (noise, potential): see GenParams
  int ppitch;             // row pitch (cells) of the POTENTIAL array: zpitch rounded up to even for float32 plans, so that the
                          // generation pass stores a cell pair (kz even, kz + 1) with one aligned 16-byte store
  // SRC = 2 kernels: the same deviates as float32 pairs (g_re, g_im), read where the one-pass replay left them -- every
  // MT19937 segment's accepted pairs densely from slot seg * seg_cap of `noise32`.  No copy into cell order: `rowtab` (built from
  // the scan of the per-segment counts by mt_rowtab_kernel, one 8-byte entry per row (ix, iy) of the stream, index iy * nx + ix so
  // that the rows of one x-pass tile are neighbours) says where a row's nz/2 + 1 consecutive stream cells start.
  const cplx<float>* noise32;
  const RowLoc* rowtab;
  unsigned long long seg_cap;          // attempts (= slots) per segment (< 2^32)
  // POT = 2 kernels: the pass emits pscale * delta(k) / k^2 instead of delta(k) -- the saved potential of generate.py:200-217
  // regenerated from the seed (or the resident deviates) when calculate_newtonian_potential asks for it, never stored
  double pscale;          // (float32 plans round it to float32, as the scaled copy of the stored potential does)
  int emit_potential;     // host side: selects those kernels
};
enum { FAST_LDS_BINS = 512 };

RF_HD float fast_log2(float t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_logf(t);   // v_log_f32
#else
  return log2f(t);
#endif
}

// rec points at the records (LDS or global)
RF_HD float fast_sigma(const FastGenParams& g, const FastRec* rec, float t /* |k|^2 */) {
  float u = fast_log2(t) * g.u_scale + g.u_off;          // (log10|k| - x0) / dx
  const float hi = (float)g.nbins - 0.001f;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __builtin_amdgcn_fmed3f(u, 0.0f, hi);              // clamp; t == 0 gives -inf -> bin 0 (a guard bin)
  const float f = __builtin_amdgcn_fractf(u);
#else
  u = fminf(fmaxf(u, 0.0f), hi);
  const float f = u - floorf(u);
#endif
  const int b = (int)u;
  const FastRec r = rec[b];
  const float d = fmaxf(f - r.fs, 0.0f);
  return (r.v0 + r.sa * f) + r.ds * d;
}

// signed fftfreq index of ix without a select: nx is a power of two, so (ix & nx/2) is 0 or nx/2
RF_HD int fast_signed_index(int ix, int nx) { return ix - 2 * (ix & (nx >> 1)); }
// kx^2 + ky^2 of column (ix, iy), and |k|^2 of its cell kz (0 <= kz <= nz/2: no wrap on the half axis)
RF_HD float fast_kxy2(const FastGenParams& g, int ix, int iy) {
  const float kx = (float)fast_signed_index(ix, g.nx) * g.dkx, ky = (float)fast_signed_index(iy, g.ny) * g.dky;
  return fmaf(kx, kx, ky * ky);
}
RF_HD float fast_k2(const FastGenParams& g, float kxy, int kz) {
  const float k = (float)kz * g.dkz;
  return fmaf(k, k, kxy);
}

// Philox counter of the cell pair (kz even, kz + 1) of column (ix, iy): half the native noise index
RF_HD uint64_t fast_pair_counter(const FastGenParams& g, int ix, int iy, int kz) {
  return (((uint64_t)ix * (uint64_t)g.ny + (uint64_t)iy) * (uint64_t)(g.nz / 2) + (uint64_t)kz) >> 1;
}

// The two packed cells kz, kz + 1 of one column from ONE Philox call: k^2 = kxy + kz2a / kz2b.
RF_HD void fast_gen_pair_at(const FastGenParams& g, const FastRec* rec, uint64_t seed, uint64_t ctr, float k2a,
                            float k2b, cplx<float>& c0, cplx<float>& c1) {
  const PhiloxOut o = philox_native(ctr, 0, seed);
  float g0, g1;
  const float s0 = fast_sigma(g, rec, k2a), s1 = fast_sigma(g, rec, k2b);
  BoxMuller<float>::run_scaled(o.w[0], o.w[1], s0, g0, g1);
  c0 = mk<float>(g0, g1);
  BoxMuller<float>::run_scaled(o.w[2], o.w[3], s1, g0, g1);
  c1 = mk<float>(g0, g1);
}
RF_HD void fast_gen_pair(const FastGenParams& g, const FastRec* rec, uint64_t seed, int ix, int iy, int kz,
                         cplx<float>& c0, cplx<float>& c1) {
  const float kxy = fast_kxy2(g, ix, iy);
  fast_gen_pair_at(g, rec, seed, fast_pair_counter(g, ix, iy, kz), fast_k2(g, kxy, kz), fast_k2(g, kxy, kz + 1), c0, c1);
}

// One packed cell with native noise index ci (float64 plans: one complex128 per lane, so the two cells of a Philox
// pair sit in neighbouring lanes; each lane runs the pair's call and keeps its own half).
RF_HD cplx<float> fast_gen_one(const FastGenParams& g, const FastRec* rec, uint64_t seed, uint64_t ci, float k2) {
  const PhiloxOut o = philox_native(ci >> 1, 0, seed);
  const bool odd = (ci & 1u) != 0;
  float g0, g1;
  BoxMuller<float>::run_scaled(odd ? o.w[2] : o.w[0], odd ? o.w[3] : o.w[1], fast_sigma(g, rec, k2), g0, g1);
  return mk<float>(g0, g1);
}

// slot kz = 0 of column (ix, iy): (plane kz=0) + i (plane kz=nz/2), each Hermitian-symmetrised
// by the rules of gen_cell() (transform.py:141-158)
RF_HD float fast_rcp(float t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(t);   // v_rcp_f32 (1 ulp)
#else
  return 1.0f / t;
#endif
}

// p0, pn: delta(k) / k^2 of the symmetrised cells kz = 0 and kz = nz/2 (0 at DC) for the save_potential store
RF_HD cplx<float> fast_fix_kz0(const FastGenParams& g, const FastRec* rec, uint64_t seed, int ix, int iy,
                               cplx<float>& p0, cplx<float>& pn) {
  const int nzc = g.nz / 2;
  const int role = sym_role(g.nx, g.ny, ix, iy);
  int sx = ix, sy = iy;
  if (role == RF_DEST) { sx = (g.nx - ix) % g.nx; sy = (g.ny - iy) % g.ny; }
  const float kxy_s = fast_kxy2(g, sx, sy);
  const uint64_t scol = (uint64_t)sx * (uint64_t)g.ny + (uint64_t)sy;
  float g0, g1;
  const float s0 = fast_sigma(g, rec, fast_k2(g, kxy_s, 0));
  const PhiloxOut os = philox_native((scol * (uint64_t)nzc) >> 1, 0, seed);
  BoxMuller<float>::run_scaled(os.w[0], os.w[1], s0, g0, g1);
  cplx<float> a = mk<float>(g0, g1);
  const float sn = fast_sigma(g, rec, fast_k2(g, kxy_s, nzc));
  const uint64_t cn = (uint64_t)g.nx * (uint64_t)g.ny * (uint64_t)nzc + scol;
  const PhiloxOut on = philox_native(cn >> 1, 0, seed);
  if (cn & 1) BoxMuller<float>::run_scaled(on.w[2], on.w[3], sn, g0, g1);
  else        BoxMuller<float>::run_scaled(on.w[0], on.w[1], sn, g0, g1);
  cplx<float> n = mk<float>(g0, g1);
  if (role == RF_DEST) { a.y = -a.y; n.y = -n.y; }
  if (role == RF_SELF) { a.y = 0.0f; n.y = 0.0f; }
  if (ix == 0 && iy == 0) a = mk<float>(0.0f, 0.0f);     // DC mode (its sigma lookup is meaningless)
  // the potential of a destination cell is the conjugate of its source's: same |k|^2 on both sides of the mirror
  const float r0 = (ix == 0 && iy == 0) ? 0.0f : fast_rcp(fast_k2(g, kxy_s, 0)), rn = fast_rcp(fast_k2(g, kxy_s, nzc));
  p0 = mk<float>(a.x * r0, a.y * r0);
  pn = mk<float>(n.x * rn, n.y * rn);
  return mk<float>(a.x - n.y, a.y + n.x);
}

// The same slot from resident deviates (the reference's stream, e.g. replayed MT19937): cell = sigma * (g_re + i g_im)
// with the float64 product rounded once (random.py:28), symmetrised as above.  SRC = 1: float64 deviates; SRC = 2: the
// float32 copies (float32 plans: the product is then formed in float32, 6e-8 relative from the once-rounded one).
// one float32 deviate pair through a GLOBAL-address-space pointer: its address comes out of selects, the compiler cannot
// infer where it points and would emit flat_load -- counted on lgkmcnt too, so that the LDS reads of the sigma lookup
// would wait for the deviates' trip to HBM
RF_HD cplx<float> load_pair_global(const cplx<float>* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 v = *(const __attribute__((address_space(1))) f2*)p;
  return mk<float>(v.x, v.y);
#else
  return *p;
#endif
}
// Where the pairs of one row of the stream live (SRC = 2).  Stream cell c = (ix ny + iy) (nz/2 + 1) + kz; the cells of segment s
// are [first[s], first[s + 1]) (exclusive scan of the per-segment counts) and sit densely from slot s * cap.  A row is nz/2 + 1
// consecutive cells, far fewer than a segment holds (the builder checks it): its first `nfirst` cells lie in segment `seg` from
// in-segment slot `off`, the others -- a segment boundary falls inside one row in a few hundred -- at the start of segment seg + 1.
// entry of the row whose first cell is c.  first: [nseg + 1] with first[nseg] = total accepted pairs.  Rows that reach beyond the
// total (a failed replay: the host reports it) point at the start of segment 0 -- in bounds, never used.  *bad is set when a row
// would span more than two segments (segments shorter than a row: the host refuses such a replay geometry).
RF_HD RowLoc make_rowloc(const unsigned long long* first, int nseg, unsigned long long c, unsigned nzh, int* bad) {
  RowLoc e;
  e.off = 0; e.seg_n = nzh;
  if (c + nzh > first[nseg]) return e;
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {                                   // largest s with first[s] <= c
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= c) lo = mid; else hi = mid - 1;
  }
  const unsigned long long left = first[lo + 1] - c;  // cells of segment lo from c on (>= 1)
  const unsigned nfirst = left < nzh ? (unsigned)left : nzh;
  if (nfirst < nzh && first[lo + 2 <= nseg ? lo + 2 : nseg] < c + nzh) *bad = 1;
  e.off = (uint32_t)(c - first[lo]);
  e.seg_n = ((uint32_t)lo << ROWLOC_NBITS) | nfirst;
  return e;
}
RF_HD RowLoc load_rowloc(const RowLoc* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  const u2 v = *(const __attribute__((address_space(1))) u2*)p;      // one global_load_dwordx2 (not a flat load: see load_pair_global)
  RowLoc e; e.off = v.x; e.seg_n = v.y;
  return e;
#else
  return *p;
#endif
}
// address of the pair of cell kz of the row
RF_HD const cplx<float>* row_pair(const FastGenParams& g, RowLoc e, int kz) {
  const uint32_t nfirst = e.seg_n & ((1u << ROWLOC_NBITS) - 1u), seg = e.seg_n >> ROWLOC_NBITS, cap = (uint32_t)g.seg_cap;
  const uint32_t slot = (uint32_t)kz < nfirst ? e.off + (uint32_t)kz : cap + ((uint32_t)kz - nfirst);
  return g.noise32 + ((unsigned long long)seg * cap + slot);
}

template <int SRC>
RF_HD cplx<float> fast_noise_cell(const FastGenParams& g, const FastRec* rec, int ix, int iy, int kz, float k2) {
  if (SRC == 2) {
    const float s = fast_sigma(g, rec, k2);
    const cplx<float> d = load_pair_global(row_pair(g, load_rowloc(g.rowtab + ((long long)iy * g.nx + ix)), kz));
    return mk<float>(s * d.x, s * d.y);
  }
  const long long c = ((long long)ix * g.ny + iy) * g.zpitch + side_slot(g, kz);
  const double* d = g.noise + 2 * c;
  const double s = (double)fast_sigma(g, rec, k2);
  return mk<float>((float)(s * d[0]), (float)(s * d[1]));
}
// p0, pn: delta(k) / k^2 of the two symmetrised cells, as fast_fix_kz0()
template <int SRC>
RF_HD cplx<float> fast_fix_kz0_noise(const FastGenParams& g, const FastRec* rec, int ix, int iy, cplx<float>& p0, cplx<float>& pn) {
  const int nzc = g.nz / 2;
  const int role = sym_role(g.nx, g.ny, ix, iy);
  int sx = ix, sy = iy;
  if (role == RF_DEST) { sx = (g.nx - ix) % g.nx; sy = (g.ny - iy) % g.ny; }
  const float kxy_s = fast_kxy2(g, sx, sy);
  cplx<float> a = fast_noise_cell<SRC>(g, rec, sx, sy, 0, fast_k2(g, kxy_s, 0));
  cplx<float> n = fast_noise_cell<SRC>(g, rec, sx, sy, nzc, fast_k2(g, kxy_s, nzc));
  if (role == RF_DEST) { a.y = -a.y; n.y = -n.y; }
  if (role == RF_SELF) { a.y = 0.0f; n.y = 0.0f; }
  if (ix == 0 && iy == 0) a = mk<float>(0.0f, 0.0f);
  const float r0 = (ix == 0 && iy == 0) ? 0.0f : fast_rcp(fast_k2(g, kxy_s, 0)), rn = fast_rcp(fast_k2(g, kxy_s, nzc));
  p0 = mk<float>(a.x * r0, a.y * r0);
  pn = mk<float>(n.x * rn, n.y * rn);
  return mk<float>(a.x - n.y, a.y + n.x);
}

// ------------------------------------------------------- c2r / r2c untangle --
// Inverse: Zc[k] = (X[k] + conj X[M-k]) + i t_k (X[k] - conj X[M-k]),  t_k = exp(+2 pi i k / N), N = 2M.
// The length-M unnormalised inverse FFT of Zc is z[m] = x[2m] + i x[2m+1] (x unnormalised, i.e. N * irfft).
template <typename T> RF_HD cplx<T> c2r_untangle(cplx<T> xk, cplx<T> xmk, cplx<T> tk) {
  cplx<T> a = mk<T>(xk.x + xmk.x, xk.y - xmk.y);
  cplx<T> d = mk<T>(xk.x - xmk.x, xk.y + xmk.y);
  cplx<T> b = cmul(tk, d);
  return mk<T>(a.x - b.y, a.y + b.x);
}
// Forward: given Z = FFT_M(z) (kernel exp(-...)), X[k] = (Z[k] + conj Z[M-k])/2 - (i/2) conj(t_k) (Z[k] - conj Z[M-k]).
template <typename T> RF_HD cplx<T> r2c_tangle(cplx<T> zk, cplx<T> zmk, cplx<T> tk) {
  cplx<T> a = mk<T>(zk.x + zmk.x, zk.y - zmk.y);
  cplx<T> d = mk<T>(zk.x - zmk.x, zk.y + zmk.y);
  cplx<T> b = cmul(cconj(tk), d);
  return mk<T>((T)0.5 * (a.x + b.y), (T)0.5 * (a.y - b.x));
}

// LDS padding: one extra slot every 16 so that stride-16 (and stride-8) write
// patterns of the first Stockham pass spread over the banks.
// LDS row image of the contiguous-axis passes: one complex of padding per 8 (a bank-conflict simulation of the
// radix-8 passes gives 1.33x the conflict-free cycles for this shift against 1.83x for one per 16)
RF_HD int pad16(int i) { return i + (i >> 3); }

}  // namespace rf
