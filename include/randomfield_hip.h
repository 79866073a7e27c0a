/*
 * randomfield_hip.h -- C-ABI of the MI355X (gfx950) Gaussian-random-field hot path.
 *
 * Drop-in boundary for the Fourier-space sampling path of dkirkby/randomfield
 * (SURVEY.md section 8b).  The reference has no FFI of its own -- the path is
 * plain Python over numpy/scipy/pyFFTW -- so each entry point below cites the
 * reference Python interface (randomfield/<file>:<line>) whose work it takes
 * over.  The Python host (randomfield_amd/) binds these with ctypes; see
 * INTEGRATION.md for the stub a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success and a non-zero status on
 * failure (message via rf_last_error(), thread-local).  No exceptions, torch
 * types or callbacks cross the boundary: plain pointers and sizes only.  A plan
 * is used from one host thread at a time.  Host arrays use the reference's
 * layouts: k-space (nx, ny, nz/2+1) complex C-order (transform.py:192), real
 * space (nx, ny, nz) dense or (nx, ny, nz+2) padded (transform.py:227-235).
 * All work is queued on the plan's HIP stream; rf_sync() waits for it.
 *
 * THIS header is the consumer surface.  Per-kernel timing, launch-structure knobs and the "virtual rank" entry points that
 * exist for tests, bench.py and the profiling tools are declared in randomfield_hip_diag.h and are not part of what a
 * consumer should bind.
 */
#ifndef RANDOMFIELD_HIP_H
#define RANDOMFIELD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rf_plan rf_plan;

enum { RF_F32 = 0, RF_F64 = 1 };                 /* complex64/float32 or complex128/float64 plan */
enum { RF_NOISE_NATIVE = 0, RF_NOISE_EXTERNAL = 1, RF_NOISE_RESIDENT = 2 };
enum { RF_LAYOUT_DENSE = 0, RF_LAYOUT_PADDED = 1 };

/* ---- library ---------------------------------------------------------- */
/* ABI version of THIS header: RF_ABI_MAJOR changes when an entry point's meaning or signature changes or one is removed, RF_ABI_MINOR on
 * every addition.  rf_version() returns the RF_ABI_VERSION the loaded library was built from: a consumer compares its major with the
 * header it was compiled against and asks rf_abi_features() which groups of entry points the build carries.  (History: rounds 1-4 of
 * this repository returned the constant 1 while the surface grew from ~20 to 70 entry points; 5.0 is the first version that means
 * something: the consumer surface below + the diagnostics of randomfield_hip_diag.h.)  rf_measure_power was added WITHOUT a new
 * minor number -- the version stays 5.5 -- and is announced by its feature bit alone: ask rf_abi_features() & RF_FEATURE_POWER_MEASURE.
 * The same holds for the second-order (2LPT) calls: rf_abi_features() & RF_FEATURE_LPT2.
 * And for the particle calls -- the resident displacement buffer and the cloud-in-cell paint, rf_particles_accumulate, rf_particles_upload,
 * rf_particles_download, rf_particles_paint: rf_abi_features() & RF_FEATURE_PARTICLES, the version stays 5.5.
 * And for rf_measure_multipoles, the redshift-space multipole moments of the binned power spectrum with an optional window compensation:
 * rf_abi_features() & RF_FEATURE_POWER_MULTIPOLES, the version stays 5.5.
 * And for the cloud-in-cell gather of a field at the particles and the shift by it -- rf_particles_gather, rf_particles_gather_download,
 * rf_particles_shift: rf_abi_features() & RF_FEATURE_PARTICLES_GATHER, the version stays 5.5.
 * And for the assignment scheme as an argument, with the triangular-shaped cloud as the second scheme -- rf_particles_paint_ex,
 * rf_particles_gather_ex: rf_abi_features() & RF_FEATURE_PARTICLES_TSC, the version stays 5.5.
 * And for the interlaced paint -- rf_particles_paint_shifted, rf_kspace_stash, rf_kspace_interlace, rf_particles_paint_interlaced:
 * rf_abi_features() & RF_FEATURE_PARTICLES_INTERLACE, the version stays 5.5.
 * And for the binned bispectrum -- rf_measure_bispectrum, rf_bispectrum_release: rf_abi_features() & RF_FEATURE_BISPECTRUM, the version
 * stays 5.5. */
#define RF_ABI_MAJOR 5
#define RF_ABI_MINOR 5
#define RF_ABI_VERSION ((RF_ABI_MAJOR << 16) | RF_ABI_MINOR)
int rf_version(void);                            /* (major << 16) | minor */
/* bit mask of the groups of entry points this build exports (each bit: every function of the group is present and works as this
 * header says; a 0 bit: calling one returns an error or the symbol is missing) */
enum {
  RF_FEATURE_REALISE = 1 << 0,             /* rf_generate / rf_execute_c2r / rf_realise / rf_realise_batch(_prepare) / rf_moments: rows K..D */
  RF_FEATURE_R2C = 1 << 1,                 /* rf_execute_r2c, rf_upload_real: the reverse plan (transform.py:278-301) */
  RF_FEATURE_C2C = 1 << 2,                 /* rf_plan_create_c2c, rf_upload_c, rf_download_c, rf_execute_c2c: Plan(packed=False) */
  RF_FEATURE_LOGNORMAL = 1 << 3,           /* rf_lognormal, rf_scale_z, rf_affine_z, rf_set_z_tables, rf_realise_lognormal: row L */
  RF_FEATURE_POTENTIAL = 1 << 4,           /* rf_realise_potential, rf_save_potential, rf_load_potential, rf_realise_scaled_potential,
                                              rf_can_regenerate_potential: generate.py:200-217, 333-347 */
  RF_FEATURE_LENSING = 1 << 5,             /* rf_lensing_potential, rf_download_aux: generate.py:352-416 */
  RF_FEATURE_MT19937 = 1 << 6,             /* rf_mt_set_jump, rf_noise_mt19937(_ex), rf_realise_batch_reference, rf_can_batch_reference:
                                              random.py:24-28 replayed on the device */
  RF_FEATURE_MT19937_SHARED = 1 << 7,      /* rf_mt_share_*: that stream shared between kz-slab ranks */
  RF_FEATURE_MULTI_RANK = 1 << 8,          /* nranks > 1 plans, rf_comm_*: kz slabs + one RCCL all-to-all (librccl is dlopen'ed by rf_comm_*) */
  RF_FEATURE_GENERIC_SHAPES = 1 << 9,      /* every even shape (axes of up to 8192 complex64 / 4096 complex128 points, or two factors that fit): rf_shape_supported(_dtype) == 2 */
  RF_FEATURE_EXCHANGE_CHUNKS = 1 << 10,    /* RF_FLAG_EXCHANGE_CHUNKS */
  RF_FEATURE_DIRECT_EXCHANGE = 1 << 12,    /* rf_comm_enable_direct: the y pass stores into the peers' receive buffers (IPC-mapped), no all-to-all kernels */
  RF_FEATURE_DIAGNOSTICS = 1 << 11,        /* the entry points of randomfield_hip_diag.h (timing per kernel, launch structure, virtual ranks) */
  RF_FEATURE_GENERIC_FUSED = 1 << 13,      /* RF_FLAG_FUSED_GENERIC_GENERATION; rf_kernel_ms on generic plans */
  RF_FEATURE_GRADIENT = 1 << 14,           /* rf_load_gradient, rf_execute_gradient_c2r: the vector field of the saved potential */
  RF_FEATURE_POWER_MEASURE = 1 << 15,      /* rf_measure_power: the binned power spectrum of the k buffer or of the field */
  RF_FEATURE_LPT2 = 1 << 16,               /* rf_load_hessian, rf_execute_hessian_c2r, rf_lpt2_source, rf_lpt2_potential, RF_GRAD_FROM_POTENTIAL2:
                                              the second-order Lagrangian displacement */
  RF_FEATURE_PARTICLES = 1 << 17,          /* rf_particles_accumulate, rf_particles_upload, rf_particles_download, rf_particles_paint: the three
                                              displacement components resident on the device, painted back onto the grid (cloud in cell) */
  RF_FEATURE_POWER_MULTIPOLES = 1 << 18,   /* rf_measure_multipoles: the moments of mu^2 behind P0, P2, P4 along a grid axis, window compensation */
  RF_FEATURE_PARTICLES_GATHER = 1 << 19,   /* rf_particles_gather, rf_particles_gather_download, rf_particles_shift: the current real field
                                              interpolated at the particles (cloud in cell, the paint's adjoint), and the particles moved by it */
  RF_FEATURE_PARTICLES_TSC = 1 << 20,      /* rf_particles_paint_ex, rf_particles_gather_ex: the paint and the gather with the assignment scheme
                                              as an argument, RF_ASSIGN_CIC or RF_ASSIGN_TSC (triangular-shaped cloud, three cells per axis) */
  RF_FEATURE_PARTICLES_INTERLACE = 1 << 21, /* rf_particles_paint_shifted, rf_kspace_stash, rf_kspace_interlace, rf_particles_paint_interlaced:
                                              the paint on a grid shifted by half a cell and the two spectra combined (interlacing) */
  RF_FEATURE_BISPECTRUM = 1 << 22          /* rf_measure_bispectrum, rf_bispectrum_release: the FFT estimator of the binned bispectrum */
};
unsigned rf_abi_features(void);
const char* rf_last_error(void);
int rf_device_count(int* count);
/* is this grid shape supported by the HIP kernels?  1: tiled power-of-two kernels (nx, ny in 8..2048, nz in 16..2048);
 * 2: generic mixed-radix kernels (any other even nx, ny, nz -- the reference's own test shapes (4,6,8) and (40,60,80), transform.py:172-177;
 * single GPU, k space materialised.  An axis of up to 8192 points -- 4096 on RF_F64 plans -- is one pass; a longer one must split into two
 * factors within that cap and takes two); 0: unsupported */
int rf_shape_supported(int nx, int ny, int nz);
/* the same for ONE dtype (RF_F32 / RF_F64): what rf_plan_create(nx, ny, nz, dtype, ...) on one rank will accept -- rf_shape_supported answers
 * for complex64 plans on the generic path (one-pass axes up to 8192 points), complex128 lines hold 4096 */
int rf_shape_supported_dtype(int nx, int ny, int nz, int dtype);

/* ---- plan: replaces transform.Plan.__init__ / allocate (transform.py:10-43,170-276)
 * One device buffer of nx*ny*nz reals (== nx*ny*nz/2 complex) is the analogue of
 * the reference's single in-place buffer.  nranks/rank select the kz-slab (k space)
 * / x-slab (real space) owned by this process for multi-GPU plans (1, 0 otherwise). */
int rf_plan_create(rf_plan** plan, int nx, int ny, int nz, int dtype, int device, int nranks, int rank);
int rf_plan_destroy(rf_plan* plan);
int rf_plan_nbytes(rf_plan* plan, size_t* nbytes);          /* transform.py:221,226 nbytes_allocated */
/* plan options.  RF_FLAG_EXACT_GENERATION = 1 makes native-noise float32 realisations use the
 * reference's exact float64 rounding chain for |k| and sigma(k) instead of the fast float32 one.
 * RF_FLAG_FORCE_SLAB_PATH = 2 routes a single-rank plan through the multi-GPU slab pipeline (y pass on the
 * slab, exchange = copy of the own block, gathering z pass, pipelined batches): a test hook.
 * RF_FLAG_REPLICATED_GENERATION = 4 (multi-rank plans, native generator): no all-to-all -- every rank generates all of
 * k space on the fly, runs the full x-FFT and keeps only its own x slab; y and z passes are local.  P-fold redundant
 * x-pass arithmetic instead of the exchange: faster when few GPUs share few xGMI links (2 GPUs: one link).
 * RF_FLAG_TRANSPOSED_INTERMEDIATE = 8 (default OFF; single-GPU plans): the x pass stores its tiles as contiguous chunks into a
 * blocked scratch array of the field's size, the y pass runs in place there and the z pass gathers from it into the field
 * buffer.  Measured on MI355X: 5 % faster at 2048^3 float32, slower at 1024^3; twice the device memory.
 * RF_FLAG_YZ_SLAB_PLANES = 16 (single-GPU plans; the value is a count, not a boolean): the y and z passes run slab by slab of
 * `value` x planes, so that the z pass finds what the y pass has just written in the 256 MiB Infinity Cache; -1 (default) picks
 * slabs of about that size, 0 = whole-grid passes.
 * RF_FLAG_EXCHANGE_CHUNKS = 32 (multi-rank plans in exchange mode; the value is a count, a power of two): the rank's kz slab is
 * generated, x- and y-transformed and SENT as `value` sub-slabs, so that inside ONE realisation (one generate_delta_field call,
 * generate.py:144-230) the all-to-all of sub-slab c runs on a second stream under the forward passes of sub-slab c + 1 instead of
 * behind all of them; the gathering z pass reads ranks x value segments per row.  1 (default) = one exchange of the whole slab.
 * RF_FLAG_FUSED_GENERIC_GENERATION = 64 (default OFF; packed single-rank plans on the generic kernels, rf_shape_supported == 2; refused
 * elsewhere): rf_realise and rf_realise_batch generate the half spectrum inside the first FFT pass instead of storing it and reading
 * it back -- 5 sweeps of the half spectrum instead of 7 and no k-space array; the field and its moments are bit-identical.  As on
 * the tiled kernels, such a realisation leaves NO k space behind: rf_download_k reports "no k-space data" on a fresh plan, and an
 * array left by rf_generate / rf_upload_k stays as it was.  rf_generate, rf_execute_c2r, rf_realise_potential, rf_execute_r2c are
 * unaffected.  (A plan whose x axis is too long for one LDS line -- the four-step form -- accepts the flag and generates into a
 * scratch array instead: same contract, no saving.) */
enum { RF_FLAG_EXACT_GENERATION = 1, RF_FLAG_FORCE_SLAB_PATH = 2, RF_FLAG_REPLICATED_GENERATION = 4, RF_FLAG_TRANSPOSED_INTERMEDIATE = 8,
       RF_FLAG_YZ_SLAB_PLANES = 16, RF_FLAG_EXCHANGE_CHUNKS = 32, RF_FLAG_FUSED_GENERIC_GENERATION = 64 };
int rf_plan_set_flag(rf_plan* plan, int flag, int value);
/* run on a caller-owned HIP stream (hipStream_t passed as void*); NULL restores the plan's own stream */
int rf_plan_set_stream(rf_plan* plan, void* hip_stream);

/* ---- inputs ----------------------------------------------------------- */
/* Per-axis float64 tables k_a(i)^2 computed by the host exactly as
 * powertools.create_ksq_grids (powertools.py:27-37): lengths nx, ny, nz/2+1. */
int rf_set_kgrid(rf_plan* plan, const double* kx2, const double* ky2, const double* kz2);
/* float64 tables x_i = log10 k_i and s_i = N3*sqrt(P_i/(2 Vbox)) computed by the host
 * exactly as powertools.tabulate_sigmas (powertools.py:153-154), n >= 2 rows. */
int rf_set_power(rf_plan* plan, const double* log10k, const double* sigma, int n);

/* ---- rows K,T,R,S: fill_with_log10k + tabulate_sigmas + randomize + symmetrize
 * (powertools.py:40-61,125-164; random.py:12-29; transform.py:114-158).
 * Leaves the symmetrised k-space array in the plan's API-layout k buffer.
 * mode RF_NOISE_NATIVE: counter-based Philox4x32-7 + Box-Muller keyed by (seed, cell).
 * mode RF_NOISE_EXTERNAL: noise_host = 2*nx*ny*(nz/2+1) float64 deviates in the order of
 * RandomState(seed).normal(size=2*M) (random.py:24-28) -- the same-seed parity mode.
 * mode RF_NOISE_RESIDENT: the deviates already in the plan's device buffer (rf_noise_mt19937 or a
 * previous external-noise call). */
int rf_generate(rf_plan* plan, uint64_t seed, int mode, const double* noise_host);

/* ---- on-GPU replay of the reference's noise stream: np.random.RandomState(seed).normal(size=2*M)
 * (random.py:24-28) = MT19937 + legacy polar method, filled into the plan's device noise buffer in the
 * reference's order; afterwards rf_generate / rf_realise with mode RF_NOISE_RESIDENT use it (same-seed
 * parity without drawing 2*M deviates on the host and uploading them).
 * rf_mt_set_jump: the jump polynomials of a radix-R tree over the segments (L = 624*blocks_per_segment words each):
 * row t*(R-1) + (m-1) holds the positions of the set coefficients of t^(m * R^t * L) mod phi(t), m = 1 .. R-1, for
 * as many stages t as the largest grid needs (computed by randomfield_amd/mt19937.py); pos is npolys x stride uint16.
 * rf_noise_mt19937: state624 = the generator's initial state (init_genrand(seed)); *accepted (may be NULL)
 * receives the number of accepted polar attempts that were generated. */
int rf_mt_set_jump(rf_plan* plan, int npolys, const uint16_t* pos, const int* npos, int stride, int blocks_per_segment, int radix);
int rf_noise_mt19937(rf_plan* plan, const uint32_t* state624, unsigned long long* accepted);
/* single = 1 (a request, honoured by float32 plans that have the fast generation pass; others keep float64): keep the
 * deviates as float32 pairs instead -- half the memory traffic of the replay and of
 * the generation pass that reads them; accept / reject stays in float64, f = sqrt(-2 log r2 / r2) is formed in float32
 * (1e-7 relative); the pairs stay in the replay's per-segment runs (8 bytes per polar attempt of the whole stream) and the
 * generation pass locates them.  rf_realise / rf_realise_potential with RF_NOISE_RESIDENT use whichever copy is resident; rf_generate,
 * rf_download_noise and float64 plans need the float64 ones (single = 0, = rf_noise_mt19937). */
int rf_noise_mt19937_ex(rf_plan* plan, const uint32_t* state624, unsigned long long* accepted, int single);
/* n same-seed realisations back to back (random.py:24-28 for each seed; single-GPU complex64 plans on the fast generation path):
 * the replay of seed i + 1 runs on a second stream under the y / z passes of seed i.  states = n x 624 words (MT19937 start
 * states, e.g. numpy's init_genrand / init_by_array of each seed); rms_out (n, optional) = np.std of every field.  The field of
 * the last seed is the plan's current field; every field equals what rf_noise_mt19937_ex(single) + rf_realise(RESIDENT) gives. */
int rf_realise_batch_reference(rf_plan* plan, const uint32_t* states, int n, double* rms_out);
/* does rf_realise_batch_reference serve this plan as it stands (single-GPU complex64 plan on the fast generation path, tables and
 * jump polynomials set, segments long enough for the float32 form)?  With n = 1 it is also the fastest way to ONE same-seed field --
 * replay and passes queued back to back, no host synchronisation between them -- and what Generator(rng='reference') calls
 * (generate.py:191-199 with random.py:24-28 inside).  1 / 0. */
int rf_can_batch_reference(rf_plan* plan);
/* ---- the same stream shared between the ranks of a kz-slab job (random.py:24-28 is ONE sequential stream; the reference is
 * single-process, so there is no reference interface to mirror beyond that definition).  rf_noise_mt19937_ex on a multi-rank
 * plan replays the whole stream on every rank; these calls replay 1/P of it per rank and exchange the deviates once:
 *   rf_mt_share_segments  the stream's segment count and this rank's range [first, first + count)
 *   rf_mt_share_begin     jump to segment `first`, replay the local segments; counts_out[count] = accepted pairs per segment
 *   rf_mt_share_gather    every rank's counts into counts_all[nseg_total], in segment order (an integer all-reduce over RCCL;
 *                         virtual ranks: concatenate on the host instead)
 *   rf_mt_share_pack      scan counts_all, pack the local pairs by destination rank
 *   rf_mt_share_exchange  one all-to-all over RCCL on the plan's stream (rf_comm_init first); rf_mt_share_exchange_local
 *                         (randomfield_hip_diag.h): the same between n virtual ranks living on one device (tests)
 *   rf_mt_share_finish    the plan's resident float64 deviates are this rank's planes of the stream (then RF_NOISE_RESIDENT)
 * single = 1 (complex64 plans): pairs travel as float32 (8 B per cell, the volume of the field's own exchange), rounded as
 * rf_noise_mt19937_ex(single = 1) rounds them; single = 0: the exact float64 deviates, bit for bit those of the replicated replay. */
int rf_mt_share_segments(rf_plan* plan, int* nseg_total, int* seg_first, int* seg_count);
int rf_mt_share_begin(rf_plan* plan, const uint32_t* state624, int single, unsigned long long* counts_out);
int rf_mt_share_gather(rf_plan* plan, unsigned long long* counts_all);
int rf_mt_share_pack(rf_plan* plan, const unsigned long long* counts_all);
int rf_mt_share_exchange(rf_plan* plan);
int rf_mt_share_finish(rf_plan* plan, unsigned long long* accepted);

/* calculate_newtonian_potential (generate.py:333-343) without a stored potential: the inverse transform of scale * delta(k) / k^2
 * with delta(k) regenerated inside the generation pass exactly as rf_realise(seed, mode) produces it (native generator: keyed by
 * (seed, cell); RF_NOISE_RESIDENT: the replayed stream still on the device).  rf_can_regenerate_potential: 1 if the plan and
 * mode allow it (fast generation pass; float32 replayed deviates), else use rf_realise_potential + rf_load_potential.
 * factor_z (optional): plane z of the result times factor_z[z], the light-cone weighting G(z)/(1+z) of generate.py:344-347, applied
 * in the z pass's store (= rf_scale_z on the finished field, without its sweep). */
int rf_can_regenerate_potential(rf_plan* plan, int mode);
int rf_realise_scaled_potential(rf_plan* plan, uint64_t seed, int mode, double scale, const double* factor_z /* nz, or NULL */);

/* ---- row X: Plan.execute (transform.py:303-315) ------------------------- */
int rf_execute_c2r(rf_plan* plan);               /* k buffer -> real field, numpy normalisation 1/(nx ny nz) */
int rf_execute_r2c(rf_plan* plan);               /* real field -> k buffer, unnormalised (transform.py:278-301's reverse plan); on a multi-rank
                                                  * plan: rows on the x slab, the all-to-all in the other direction, columns on the kz slab */

/* ---- unpacked complex-to-complex plans: Plan(packed=False) (transform.py:207-213,266-270; the reference's
 * tests/test_transform.py:180-298).  One device buffer [nx][ny][nz] complex, transformed in place.
 * Power-of-two axes in [8, 2048] run on the tiled kernels, any other even axes on the generic ones (up to 8192 (RF_F32) / 4096 (RF_F64) points in one pass, longer ones split into two factors that fit).
 * Only rf_upload_c / rf_download_c / rf_execute_c2c,
 * rf_sync, rf_elapsed_ms, rf_plan_set_stream, rf_plan_nbytes, rf_device_ptr and rf_plan_destroy apply. */
int rf_plan_create_c2c(rf_plan** plan, int nx, int ny, int nz, int dtype, int device);
int rf_upload_c(rf_plan* plan, const void* host);     /* [nx][ny][nz] complex64 / complex128, C order */
int rf_download_c(rf_plan* plan, void* host);
/* direction = -1: forward, unnormalised (np.fft.fftn); +1: inverse with numpy's 1/(nx ny nz) (np.fft.ifftn) */
int rf_execute_c2c(rf_plan* plan, int direction);

/* ---- fused K,T,R,S,X,D: Generator.generate_delta_field(save_potential=False)
 * (generate.py:191-199,218-219).  Generation is fused into the first FFT pass; the
 * k-space array is never materialised.  rms/mean are available from rf_moments(). */
int rf_realise(rf_plan* plan, uint64_t seed, int mode, const double* noise_host);
/* The reference's DEFAULT call, generate_delta_field(save_potential=True) (generate.py:191-219): as rf_realise, and
 * delta(k) / k^2 (0 at DC; generate.py:200-217) is left in the plan's potential buffer for rf_load_potential (on a kz-slab
 * rank: its own planes, then the Nyquist plane).  With the native generator (float32 and float64 plans) or resident float32
 * deviates (rf_noise_mt19937_ex(single), float32 plans) the potential is a second store stream of the generation pass and
 * delta(k) is never materialised; otherwise (host deviates, exact-generation flag, generic shapes) the call runs
 * rf_generate -> rf_save_potential -> rf_execute_c2r. */
int rf_realise_potential(rf_plan* plan, uint64_t seed, int mode, const double* noise_host);
/* n realisations back to back (native noise); the field of the last seed stays resident; rms_out[i]
 * (may be NULL) = np.std of field i.  Single-GPU plans replay one captured hipGraph.  Multi-GPU plans
 * pipeline instead: realisation i+1's generation / x / y passes run on the compute stream while
 * realisation i's all-to-all is in flight on a second stream (two buffer pairs). */
int rf_realise_batch(rf_plan* plan, const uint64_t* seeds, int n, double* rms_out);
/* capture + instantiate the n-realisation graph now (otherwise the first rf_realise_batch(n) does it) */
int rf_realise_batch_prepare(rf_plan* plan, int n);

/* ---- row D: np.std(delta.flat) (generate.py:219) ------------------------ */
int rf_moments(rf_plan* plan, double* mean, double* std);

/* ---- row L: cosmotools.apply_lognormal_transform (cosmotools.py:206-221) and the
 * per-z scaling delta *= mean_matter_density (generate.py:273).
 * a_z[iz] = sqrt(log t), b_z[iz] = sqrt(t), t = 1 + (sigma*growth[iz])^2 (host, float64);
 * field <- exp(field / sigma * a_z) / b_z with the reference's four roundings. */
int rf_lognormal(rf_plan* plan, const double* a_z, const double* b_z, int nz, double sigma);
/* The same two rows fused into the realisation (single-GPU plans, power-of-two axes): generate_delta_field(save_potential=False)
 * followed by convert_delta_to_density(apply_lognormal_transform=True) (generate.py:191-199,218-219,266-273) as ONE call of five
 * sweeps.  sigma = np.std(delta) (generate.py:219) is obtained before the last pass from the y pass's output (Parseval; the mean
 * is 0 because the DC mode is), the tables are formed on the device and the map runs in the z pass's epilogue as
 * exp(delta * (a_z / sigma)) * (density_z / b_z): within a few ulp of exp's argument of the reference's four statements (1e-15
 * relative for float64 fields; rf_lognormal / rf_scale_z are the rounding-exact, unfused forms).  rf_set_z_tables: growth_z (nz) and, optionally, the mean-density factor (generate.py:273),
 * once per plan.  *sigma_out (optional; blocks) = the rms of the Gaussian field; rf_moments afterwards describes the DENSITY. */
int rf_set_z_tables(rf_plan* plan, const double* growth_z, const double* density_z_or_null, int nz);
int rf_realise_lognormal(rf_plan* plan, uint64_t seed, int mode, const double* noise_or_null, double* sigma_out);
int rf_scale_z(rf_plan* plan, const double* factor_z, int nz);
/* field <- field * mul_z[iz] + add (generate.py:271-272 non-lognormal branch) */
int rf_affine_z(rf_plan* plan, const double* mul_z, int nz, double add);

/* ---- save_potential branch (generate.py:200-217, 333-343) ---------------- */
/* potential(k) = delta(k) / k^2 (0 at DC) from the k buffer into the plan's second k buffer */
int rf_save_potential(rf_plan* plan);
/* k buffer <- scale * potential(k)  (then rf_execute_c2r gives the Newtonian potential) */
int rf_load_potential(rf_plan* plan, double scale);

/* ---- gradient of the saved potential: displacement / velocity components -- */
/* psi_a(k) = i k_a delta(k) / k^2, a = axis in {0, 1, 2} (x, y, z), so that div psi = -delta: the vector field the saved potential
 * is kept for.  k_a = dk * m, m the signed mode number of the cell along the axis and dk = 2 pi / (n_axis * spacing) (the caller's);
 * m = 0 at the axis' own Nyquist index, where i k is not Hermitian: that plane and the DC cell are exactly 0.  The factor
 * scale * dk * m is formed in float64 and rounded once to the plan's real type.
 * source = RF_GRAD_FROM_POTENTIAL: from the stored potential (rf_save_potential / rf_realise_potential), which is left as it is;
 * source = RF_GRAD_FROM_KSPACE: from the k buffer holding delta(k) -- the factor takes the 1 / k^2, summed in float64 from the
 * tables of rf_set_kgrid -- for plans that regenerate their potential instead of storing it;
 * source = RF_GRAD_FROM_POTENTIAL2 (RF_FEATURE_LPT2): from the second-order potential of rf_lpt2_potential, read exactly as
 * RF_GRAD_FROM_POTENTIAL reads the stored one; refused ("no second-order potential") unless that call has run since the stored
 * potential was last written.
 * Packed single-rank plans, tiled and generic; c2c plans, nranks > 1, another axis and a missing source are refused, nothing queued. */
enum { RF_GRAD_FROM_POTENTIAL = 0, RF_GRAD_FROM_KSPACE = 1, RF_GRAD_FROM_POTENTIAL2 = 2 };
/* k buffer <- psi_a(k) (RF_GRAD_FROM_KSPACE: in place); rf_download_k and rf_execute_c2r then work as usual */
int rf_load_gradient(rf_plan* plan, int axis, double scale, double dk, int source);
/* the real field psi_a(x) in place of the current one, moments as after rf_execute_c2r.  Generic plans apply the factor inside their
 * x pass (no sweep of its own; the field is that of rf_load_gradient + rf_execute_c2r bit for bit), tiled plans run those two steps.
 * The k buffer afterwards: RF_GRAD_FROM_KSPACE consumes it (no k-space data until the next generate / upload / load);
 * RF_GRAD_FROM_POTENTIAL leaves what it held (generic plans) or psi_a(k) (tiled plans). */
int rf_execute_gradient_c2r(rf_plan* plan, int axis, double scale, double dk, int source);

/* ---- second-order (2LPT) displacement (rf_abi_features() & RF_FEATURE_LPT2) -- */
/* H_ab(k) = D_a D_b phi(k) = -scale (dk_a m_a)(dk_b m_b) phi(k), 0 <= a <= b <= 2: one component of the Hessian of the potential, D the
 * spectral derivative of rf_load_gradient (m = 0 at index 0 and at the axis' own Nyquist index, on the diagonal a = b too, so that H_ab
 * is the gradient applied twice).  Cells with m_a m_b = 0 -- the DC cell among them -- are exactly 0.  The real factor is formed in
 * float64 (and divided by k^2 from the tables of rf_set_kgrid when the source is delta(k)) and rounded once to the plan's real type.
 * source: RF_GRAD_FROM_POTENTIAL or RF_GRAD_FROM_KSPACE, state handling as rf_load_gradient.
 * Packed single-rank plans, tiled and generic; c2c plans, nranks > 1, axes outside 0..2, a > b and a missing source are refused, nothing
 * queued. */
/* k buffer <- H_ab(k) (RF_GRAD_FROM_KSPACE: in place) */
int rf_load_hessian(rf_plan* plan, int a, int b, double scale, double dk_a, double dk_b, int source);
/* the real field H_ab(x) in place of the current one; generic plans apply the factor inside their x pass (the field is that of
 * rf_load_hessian + rf_execute_c2r bit for bit), tiled plans run those two steps.  Moments and the k buffer afterwards: as
 * rf_execute_gradient_c2r. */
int rf_execute_hessian_c2r(rf_plan* plan, int a, int b, double scale, double dk_a, double dk_b, int source);
/* The source of the second-order potential, S(x) = sum over a < b of H_aa H_bb - H_ab^2 with scale = 1, from the STORED potential
 * (rf_save_potential / rf_realise_potential; only read, bit-identical afterwards): six Hessian transforms in the order xx, yy, zz, xy,
 * xz, yz, each followed by one elementwise sweep in the plan's real type (fused multiply-adds, no atomics: the same bits on every
 * call).  dk[3] = 2 pi / (n_a * spacing) per axis.  S(x) becomes the current real field (rf_download_real); its moments are not
 * computed (rf_moments refuses until the next transform); the k buffer holds no k-space data afterwards.  The first call allocates
 * two arrays of the field's size for the accumulators (counted by rf_plan_nbytes, freed with the plan). */
int rf_lpt2_source(rf_plan* plan, const double* dk);
/* phi2(k) = rfftn(S)(k) / k^2, 0 at DC, k^2 as rf_save_potential forms it: rf_lpt2_source, the forward transform as rf_execute_r2c,
 * the division -- into the accumulators' memory, in the stored potential's layout.  Afterwards the k buffer holds S(k), the field buffer
 * is as rf_execute_r2c leaves it, and rf_load_gradient / rf_execute_gradient_c2r take RF_GRAD_FROM_POTENTIAL2:
 * psi2_a(x) = rf_execute_gradient_c2r(a, 3/7, dk_a, RF_GRAD_FROM_POTENTIAL2), so that x = q + D1 psi1 + D1^2 psi2 (D2 = -3/7 D1^2).
 * The second-order potential is dropped by everything that writes the stored one (rf_save_potential, rf_realise_potential) and by the
 * next rf_lpt2_source.  Needs rf_set_kgrid. */
int rf_lpt2_potential(rf_plan* plan, const double* dk);

/* ---- particles: resident displacements and the cloud-in-cell paint (rf_abi_features() & RF_FEATURE_PARTICLES) -- */
/* One particle of unit mass per lattice cell q = (ix, iy, iz).  Its displacement s_a(q), a = 0, 1, 2, in length units lives in a buffer
 * Q[3][nx][ny][nz] of the plan's real type, allocated (and zeroed) by the first of these calls together with nothing else; the paint adds
 * an accumulator grid of 8 bytes per cell.  Both are counted by rf_plan_nbytes and freed with the plan.  Packed single-rank plans, tiled
 * and generic; c2c plans and nranks > 1 are refused, nothing queued.  No call here touches the k buffer, the stored potential or the
 * second-order potential. */
/* Q_axis = (first ? 0 : Q_axis) + coeff * W, W the current real field, which is left as it is: one elementwise sweep, coeff rounded once
 * to the plan's real type, then one product (first) or one fused multiply-add per cell -- no atomics, the same bits on every call.
 * x = q + D1 psi1 + D1^2 psi2: rf_execute_gradient_c2r(a, 1, dk_a, RF_GRAD_FROM_POTENTIAL), rf_particles_accumulate(a, D1, 1), then
 * rf_execute_gradient_c2r(a, 3/7, dk_a, RF_GRAD_FROM_POTENTIAL2), rf_particles_accumulate(a, D1 * D1, 0). */
int rf_particles_accumulate(rf_plan* plan, int axis, double coeff, int first);
/* one component, a dense [nx][ny][nz] array of the plan's real type, from / to the host (blocking) */
int rf_particles_upload(rf_plan* plan, int axis, const void* host);
int rf_particles_download(rf_plan* plan, int axis, void* host);
/* Cloud-in-cell mass assignment of the displaced particles; delta_cic becomes the current real field (rf_download_real,
 * rf_measure_power(RF_POWER_FROM_FIELD)), its moments are not computed (rf_moments refuses until the next transform).  inv_h[a] =
 * 1 / (grid spacing along a), positive and finite.  Per axis, in float64: u = (double)s_a * inv_h[a] (one rounded product), c = floor(u),
 * t = floor((u - c) * 65536) in [0, 65535] (for -2^-54 <= u < 0 alone u - c rounds to 1 and t = 65536); the weights 65536 - t and t go to the cells j0 = (i_a + c) mod n_a -- the mod formed in
 * float64 before any conversion to integer, so every finite u lands inside the grid -- and j1 = (j0 + 1) mod n_a.  The eight products of
 * three weights (exact, summing to 2^48 per particle) are added to an unsigned 64-bit grid A with integer atomics: A, and with it the
 * field, is the same bit for bit on every call, whichever kernel form runs.  delta_cic = (double)A * 2^-48 - 1, rounded once to the plan's
 * real type.  A particle whose u is not finite on some axis (a NaN or infinite displacement) adds nothing; *dropped is their number.
 * LIMIT: fewer than 65536 (2^64 / 2^48) particles' worth of mass may land in one cell; beyond it A wraps around, undetected.  Gaussian
 * initial conditions stay orders of magnitude below.  Blocks until *dropped is on the host. */
int rf_particles_paint(rf_plan* plan, const double* inv_h, unsigned long long* dropped);

/* ---- particles: a field gathered at the particles, and the shift by it (rf_abi_features() & RF_FEATURE_PARTICLES_GATHER) -- */
/* The paint's adjoint: the current real field W (dense [nx][ny][nz], the plan's real type T) interpolated with cloud-in-cell weights at
 * the displaced particles.  The values live in a buffer G[3][nx][ny][nz] of T indexed by the particle's LATTICE cell, as Q is -- three
 * slots, so the three components of a vector field can be gathered at the same positions before any of them moves the particles.  G is
 * allocated (and zeroed) by the first rf_particles_gather, counted by rf_plan_nbytes and freed with the plan.  Same plans as above; c2c
 * plans and nranks > 1 are refused, nothing queued.
 *
 * For the particle of cell q the indices j0 / j1 and the integer weights w0 / w1 (w0 + w1 = 65536) per axis are exactly those of
 * rf_particles_paint.  Everything that follows is float64, every product and every sum rounded on its own (nothing fused):
 *   v(cx,cy,cz) = (double) W[jx_cx][jy_cy][jz_cz]
 *   a(cx,cy)    = (double)wz0 * v(cx,cy,0) + (double)wz1 * v(cx,cy,1)
 *   b(cx)       = (double)wy0 * a(cx,0)    + (double)wy1 * a(cx,1)
 *   g           = ((double)wx0 * b(0) + (double)wx1 * b(1)) * 2^-48
 *   G_slot[q]   = first ? (T)(coeff * g) : (T)((double)G_slot[q] + coeff * g)          one rounding to T
 * No atomics: the same bits on every call, whichever kernel form runs.  Zero weights are NOT skipped: a non-finite value of W reaches
 * every particle whose eight cells contain it, also where its weight is zero.  A particle whose u is not finite on some axis gathers
 * g = 0 -- `first` writes 0, otherwise G_slot[q] stays -- and *dropped is the number of such particles.  For an integer-valued W the sum
 * of g 2^48 over the particles equals the sum over the cells of A W, A the paint's grid of the same displacements, exactly.
 * Reads the current real field (what rf_particles_accumulate reads) and changes nothing but G_slot: the field, Q, the paint's grid, the
 * k buffer, both potentials and the moments stay bit for bit.  Blocks until *dropped is on the host. */
int rf_particles_gather(rf_plan* plan, const double* inv_h, int slot, double coeff, int first, unsigned long long* dropped);
/* one slot, a dense [nx][ny][nz] array of the plan's real type, to the host (blocking); refused before the first gather */
int rf_particles_gather_download(rf_plan* plan, int slot, void* host);
/* Q_axis = fma(coeff, G_slot, Q_axis): the sweep of rf_particles_accumulate(first = 0) with the gathered values in the field's place --
 * coeff rounded once to T, one fused multiply-add per particle.  Refused without displacements or before the first gather. */
int rf_particles_shift(rf_plan* plan, int axis, int slot, double coeff);

/* ---- particles: the assignment scheme as an argument; triangular-shaped cloud (rf_abi_features() & RF_FEATURE_PARTICLES_TSC) -- */
/* The scheme's value is its window order p: the power of sinc that rf_measure_multipoles' window compensation divides out of a field
 * painted with it. */
enum { RF_ASSIGN_CIC = 2, RF_ASSIGN_TSC = 3 };
/* rf_particles_paint and rf_particles_gather with the scheme as an argument of the call (no plan state): RF_ASSIGN_CIC is those calls
 * word for word; any scheme but these two is refused with nothing queued.  The kernel form chosen with the diagnostics' set-form calls
 * applies to both schemes.  RF_ASSIGN_TSC, per axis: u, the drop rule, c = floor(u), t in [0, 65536] and j0 exactly as for cloud in cell;
 * then, in integers,
 *   up = t >= 32768,  tau = up ? t - 32768 : t + 32768 in [0, 65535]   (tau / 65536: the offset from the left edge of the nearest cell)
 *   jc = up ? (j0 + 1) mod n : j0,  jm = (jc - 1) mod n,  jp = (jc + 1) mod n      (two coincide on an axis shorter than three cells)
 *   Wm = (65536 - tau)^2 >> 17,  Wp = tau^2 >> 17,  W0 = 65536 - Wm - Wp            (64-bit arithmetic)
 * -- (1 - s)^2 / 2, 1/2 + s - s^2, s^2 / 2 at s = tau / 65536 to within 1, 2 and 1 units of 2^-16; the three sum to 65536 and
 * Wp - Wm = tau - 32768 exactly.  Paint: the 27 products W_x W_y W_z (exact, 2^48 per particle) are added to the same grid A with integer
 * atomics, zero products skipped; delta, rf_particles_download_counts and the LIMIT of rf_particles_paint are unchanged, and the field
 * is the same bit for bit on every call and kernel form.  Gather: float64, every product and sum rounded on its own,
 *   lerp3(w, v) = ((double)w_m * v_m + (double)w_0 * v_0) + (double)w_p * v_p
 * along z first, then y, then x, times 2^-48, then G_slot[q] exactly as rf_particles_gather forms it; zero weights are NOT skipped, a
 * dropped particle gathers 0.  For an integer-valued W the adjoint identity of rf_particles_gather holds with the TSC paint's A.
 * Pass window order 3 ('tsc') to the window compensation of a measurement of a TSC-painted field. */
int rf_particles_paint_ex(rf_plan* plan, const double* inv_h, int scheme, unsigned long long* dropped);
int rf_particles_gather_ex(rf_plan* plan, const double* inv_h, int scheme, int slot, double coeff, int first, unsigned long long* dropped);

/* ---- particles: the interlaced paint (rf_abi_features() & RF_FEATURE_PARTICLES_INTERLACE) -- */
/* Interlacing (Sefusatti et al. 2016): the particles are painted a second time on a grid shifted by half a cell on every axis, and the
 * two spectra are combined with the phase that undoes the shift; every aliased image with an odd sum of image indices cancels.
 * rf_particles_paint_shifted: rf_particles_paint_ex with the shift as an argument.  half_cell = 0 is that call word for word; 1 paints
 * the particle at u + 1/2 on all three axes; anything else is refused with nothing queued.  Per axis u, the drop rule (decided on u,
 * before the shift), c, t in [0, 65536], j0 and j1 exactly as for cloud in cell; then, in integers (the shift is exact in 2^-16 units),
 *   t2 = t + 32768,  carry = t2 >= 65536,  t' = carry ? t2 - 65536 : t2 in [0, 65535]     (t = 65536 gives t' = 32768 with a carry)
 *   j0' = carry ? j1 : j0,  j1' = (j0' + 1) mod n        (on the wrapped index: it steps for every finite u)
 *   w0' = 65536 - t',  w1' = t'
 * and RF_ASSIGN_TSC takes (t', j0') where it took (t, j0).  Counts, delta, rf_particles_download_counts, the LIMIT of
 * rf_particles_paint and "the same bits on every call and kernel form" are unchanged.  There is no shifted gather.
 * rf_kspace_stash: S <- K, S a lazy second half spectrum of K's size and layout (counted by rf_plan_nbytes, freed with the plan, never
 * stale before that: it is the caller's data).  Refused without k-space data.
 * rf_kspace_interlace: K <- (S + p K) / 2 per cell, p = px[ix] py[iy] pz[iz]; S stays valid.  px, py, pz: nx, ny, nz/2 + 1 complex
 * float64 entries as interleaved (re, im) pairs on the host, NULL = all ones; a non-finite entry is refused.  All in float64, every
 * product and sum rounded on its own:
 *   a = px py   (ar = xr yr - xi yi,  ai = xr yi + xi yr),   p = a pz,   q = p (double)K   (the same form),
 *   K = (T)(0.5 ((double)S + q))  per component, one rounding to the plan's type.
 * Refused without a stash ("no stashed spectrum") or without k-space data.  The tables that undo the half-cell shift are
 * p_a[i] = exp(+i pi m / n_a), m the signed mode number of index i, with p_a[0] = 1 and p_a[n_a / 2] = 0 (the Hermitian part of
 * exp(+-i pi / 2): the combined spectrum stays Hermitian, and the planes at an axis' own Nyquist index hold half the first spectrum).
 * rf_particles_paint_interlaced: the whole sequence -- paint (half_cell = 0), forward transform, stash, paint (half_cell = 1), forward
 * transform, combine, rf_execute_c2r.  Afterwards K holds the interlaced spectrum (valid k-space data: RF_POWER_FROM_KSPACE reads it
 * without a further transform), the current field is its inverse transform with moments as after any c2r, A holds the SHIFTED paint's
 * counts, and *dropped is the first paint's count (the second's equals it; the call blocks for it once, at its end).  The first transform writes its spectrum straight into S.
 * rf_elapsed_ms covers the whole call; rf_kernel_ms is refused after it.
 * Packed single-rank plans, tiled and generic, both dtypes.  c2c plans, nranks > 1, missing displacements, a bad scheme or half_cell and
 * a non-finite table entry are refused with nothing queued.  Q, G, the stored potential and the second-order potential are never touched. */
int rf_particles_paint_shifted(rf_plan* plan, const double* inv_h, int scheme, int half_cell, unsigned long long* dropped);
int rf_kspace_stash(rf_plan* plan);
int rf_kspace_interlace(rf_plan* plan, const double* px, const double* py, const double* pz);
int rf_particles_paint_interlaced(rf_plan* plan, const double* inv_h, int scheme, const double* px, const double* py, const double* pz,
                                  unsigned long long* dropped);

/* ---- binned power spectrum (rf_abi_features() & RF_FEATURE_POWER_MEASURE) -- */
/* The estimator that closes P(k) -> delta(x) -> P^(k): one sweep of the half spectrum [nx][ny][nz/2+1] of unnormalised forward-transform
 * values, as rf_generate / rf_upload_k / rf_execute_r2c leave them.  Cell (ix, iy, iz) has k^2 = (kx2[ix] + ky2[iy]) + kz2[iz] (float64,
 * the tables of rf_set_kgrid) and the weight w = 1 on the planes iz = 0 and iz = nz/2, 2 elsewhere.  k_edges: nbins + 1 strictly
 * increasing edges in k, k_edges[0] >= 0, 1 <= nbins <= 1024; they are squared once in float64 and a cell belongs to bin b iff
 * e2[b] <= k^2 < e2[b+1].  The DC cell and cells outside all bins are dropped.  Per bin: count = sum of w (exact), sum_k = sum of
 * w sqrt(k^2), sum_p = sum of w |delta(k)|^2, values widened to float64 and summed in float64 in a fixed order: the same plan, data and
 * edges give the same bits on every call.  With N = nx ny nz and V = N spacing^3: k = sum_k / count, P = (V / N^2) sum_p / count.
 * source = RF_POWER_FROM_KSPACE reads the k buffer and changes nothing.  source = RF_POWER_FROM_FIELD transforms the current field first:
 * generic plans as rf_execute_r2c does (the field stays, the k buffer then holds delta(k)); tiled plans run the forward passes in place
 * and sweep the packed array directly -- no k-space array is allocated or written, the field is consumed as by rf_execute_r2c, the k
 * buffer and its validity stay as they were, and the sums differ from rf_execute_r2c + RF_POWER_FROM_KSPACE by summation order only.
 * Packed single-rank plans, tiled and generic, both dtypes; c2c plans, nranks > 1, a missing kgrid, bad edges and a missing source are
 * refused with nothing queued.  Blocks until the three arrays (nbins entries each) are on the host; rf_elapsed_ms covers the call. */
enum { RF_POWER_FROM_KSPACE = 0, RF_POWER_FROM_FIELD = 1 };
int rf_measure_power(rf_plan* plan, int source, const double* k_edges, int nbins, unsigned long long* count, double* sum_k, double* sum_p);

/* ---- power spectrum multipoles (rf_abi_features() & RF_FEATURE_POWER_MULTIPOLES) -- */
/* The same sweep with a line of sight along grid axis los_axis (0, 1, 2: plane-parallel) and an optional window compensation.  Cells, k^2,
 * bins, weights w, source, preconditions, blocking and rf_elapsed_ms are exactly rf_measure_power's.  mu^2 = k_los^2 / k^2, k_los^2 the
 * entry of that axis' own table of rf_set_kgrid (one float64 division).  comp_x, comp_y, comp_z: float64 tables of nx, ny, nz/2 + 1
 * entries, each may be NULL (= all ones); c = (comp_x[ix] comp_y[iy]) comp_z[iz] and e = c |delta(k)|^2 (for a mass-assignment window
 * of order p: sinc(pi m / n)^(-2p) per axis, m the signed frequency index).  Per bin, nbins entries each: count = sum of w (exact),
 * sum_k = sum of w sqrt(k^2), m0 = sum of w e, m2 = sum of w (e mu^2), m4 = sum of w ((e mu^2) mu^2) -- moments of mu^2, every term
 * non-negative, summed in float64 in a fixed order: the same plan, data, edges and tables give the same bits on every call.  With
 * Mj = (V / N^2) mj / count the multipoles are P0 = M0, P2 = (5/2)(3 M2 - M0), P4 = (9/8)(35 M4 - 30 M2 + 3 M0).  With NULL tables
 * the terms of count, sum_k and m0 are those of rf_measure_power's count, sum_k and sum_p (the float sums agree to summation order).
 * Refused with nothing queued: what rf_measure_power refuses, a los_axis outside 0..2, and a compensation entry that is not finite and
 * positive.  The call's lazy buffer (edges, result, tables, per-workgroup partials) is counted by rf_plan_nbytes. */
int rf_measure_multipoles(rf_plan* plan, int source, int los_axis, const double* k_edges, int nbins,
                          const double* comp_x, const double* comp_y, const double* comp_z,
                          unsigned long long* count, double* sum_k, double* m0, double* m2, double* m4);

/* ---- binned bispectrum (rf_abi_features() & RF_FEATURE_BISPECTRUM) -- */
/* The FFT estimator of the bispectrum (Scoccimarro 2015; Sefusatti et al. 2016) of the half spectrum in the k buffer.  k_edges: nbins + 1
 * strictly increasing edges in k, k_edges[0] >= 0, 1 <= nbins <= 32, squared once in float64; cell (ix, iy, iz) with
 * k^2 = (kx2[ix] + ky2[iy]) + kz2[iz] belongs to shell b iff e2[b] <= k^2 < e2[b+1] and the DC cell to none: rf_measure_power's bins,
 * bit for bit.  For every shell, D_b(x) = the inverse transform (1/N, as rf_execute_c2r) of the spectrum restricted to shell b.
 * triples: ntriples x 3 bin indices, 1 <= ntriples <= 8192, every triple 0 <= b1 <= b2 <= b3 < nbins, duplicates allowed.
 *   sum3[t] = sum over all N = nx ny nz cells x of D_b1(x) D_b2(x) D_b3(x),
 * every term ((double)D1 (double)D2) (double)D3 with both products rounded on their own, the terms summed in float64 in a fixed order
 * without floating-point atomics: the same plan, data, edges and triples give the same bits on every call.  In exact arithmetic
 * N^2 sum3[t] is the sum of delta(k1) delta(k2) delta(k3) over all ORDERED triangles k_i in shell b_i with k1 + k2 + k3 = 0 modulo
 * the grid -- triangles that close only through aliasing included (none exists while the last edge is at most 2/3 of the Nyquist
 * frequency).  unit != 0: delta = 1 inside the shells, so that N^2 sum3[t] is the integer number of those triangles.  With
 * V = N spacing^3 the estimate is B = (V^2 / N^3) sum3_data / sum3_unit.
 * amp_x, amp_y, amp_z: float64 tables of nx, ny, nz/2 + 1 finite positive entries, each may be NULL (= ones): delta(k) is multiplied by
 * amp = (amp_x[ix] amp_y[iy]) amp_z[iz] in float64 and rounded once per component to the plan's type (window compensation: the square
 * roots of rf_measure_multipoles' tables); with three NULLs the kept cells are taken bit for bit.  Ignored (not even checked) when
 * unit != 0.
 * Reads the k buffer and the tables of rf_set_kgrid.  The k buffer, its validity, the stash, both potentials and the particle arrays
 * are untouched, bit for bit.  The field buffer is the transforms' workspace: afterwards there is no real-space field on any kind of
 * plan (rf_download_real refuses).  Lazy memory, counted by rf_plan_nbytes and freed by rf_bispectrum_release or with the plan: one
 * masked half spectrum (the k buffer's size), nbins shell fields (the field buffer's size each), and
 * 8 (12321 + nx + ny + nz/2 + 1 + rows ntriples) bytes of tables and per-workgroup partials, rows as rf_bispectrum_geometry
 * (randomfield_hip_diag.h) reports them; a plan that has not transformed anything yet also allocates the transforms' own scratch.
 * Packed single-rank plans, tiled and generic, both dtypes.  c2c plans, nranks > 1, RF_FLAG_FORCE_SLAB_PATH, a missing kgrid, missing
 * k-space data, bad edges, a bad triple and a bad table entry are refused with nothing queued and nothing allocated.  Blocks until
 * sum3 is on the host; rf_elapsed_ms covers the call, rf_kernel_ms gives [0] the shell filters, [1] the transforms, [2] the reduction. */
int rf_measure_bispectrum(rf_plan* plan, const double* k_edges, int nbins, const int* triples, int ntriples,
                          const double* amp_x, const double* amp_y, const double* amp_z, int unit, double* sum3);
int rf_bispectrum_release(rf_plan* plan);      /* frees the call's lazy buffers */

/* ---- host <-> device (layout conversion to/from the reference's arrays) -- */
int rf_upload_k(rf_plan* plan, const void* host);            /* (nx, ny, nz/2+1) complex */
int rf_download_k(rf_plan* plan, void* host);
int rf_upload_real(rf_plan* plan, const void* host, int layout);
/* rows x0 <= ix < x1 of the real field into host (shape (x1-x0, ny, nz) or (.., nz+2)) */
int rf_download_real(rf_plan* plan, void* host, int layout, int x0, int x1);
/* raw device pointers (real field / k buffer) for zero-copy consumers */
int rf_device_ptr(rf_plan* plan, void** real_field, void** kspace);

/* ---- lensing potential (generate.py:352-416): psi[x][y][e] = Simpson integral over iz in [i_min, e] of
 * -2 (cot_z[iz] - cot_z[e]) * field[x][y][iz] with step `spacing` (scipy.integrate.simps(even='avg') semantics),
 * 0 for e < i_min.  Reads the real field on the device, writes an auxiliary real field (the k buffer's memory:
 * any k-space data there is lost); cot_z = cotK(D) of generate.py:383-395, nz doubles. */
int rf_lensing_potential(rf_plan* plan, const double* cot_z, int nz, double spacing, int i_min);
int rf_download_aux(rf_plan* plan, void* host, int x0, int x1);   /* planes [x0, x1) of the auxiliary field, dense */

/* generate.py:184-189,230 (the reference's calls return HOST arrays): arm a host buffer (layout and size as rf_download_real's, all nx
 * planes; ordinary pageable memory) and the NEXT realisation of a single-GPU plan on the tiled kernels delivers its field there slab by
 * slab -- the device -> host copy of each slab of x planes runs as soon as that slab's z pass has finished, while the GPU works on
 * the following slabs -- and returns when the field is complete on the host.  One shot; rf_host_sink_delivered reports whether the
 * armed call delivered (else use rf_download_real) and disarms.  host = NULL disarms. */
int rf_set_host_sink(rf_plan* plan, void* host, int layout);
int rf_host_sink_delivered(rf_plan* plan, int* delivered);

/* ---- stream control and timing ------------------------------------------ */
int rf_sync(rf_plan* plan);
/* GPU time (hipEvents on the plan's stream) of the last rf_realise / rf_realise_batch /
 * rf_execute_* call, in milliseconds; blocks until that call has finished. */
int rf_elapsed_ms(rf_plan* plan, float* ms);

/* ---- multi-GPU: one process per GPU, RCCL all-to-all between the y and z passes.
 * The 128-byte unique id comes from rank 0 and is distributed by the host
 * (torch.distributed / a file / MPI ...).  No-op requirement for nranks == 1. */
int rf_comm_unique_id(void* id128);
int rf_comm_init(rf_plan* plan, const void* id128);
/* COLLECTIVE (every rank of the communicator calls it with the same `enable`).  The exchange WITHOUT send / receive kernels: the y pass
 * of every rank stores its output tiles straight into the receive buffer of the rank that owns their x planes -- the buffers are
 * mapped into the peers' address spaces once, here (hipIpcGetMemHandle / one ncclAllGather / hipIpcOpenMemHandle) -- and one tiny
 * all-reduce per realisation is the barrier between the peers' stores and the z pass.  Local HBM traffic is then what the passes
 * alone move (the grouped ncclSend / ncclRecv exchange reads every block and writes every segment once more: DESIGN.md section 5).
 * The mapping is proved with markers stored from a kernel before it is used.  *enabled = 1: all ranks switched; 0: some rank could
 * not (no IPC between these devices, a grid whose y-pass tiles straddle x planes ...) and ALL ranks keep the RCCL exchange -- that is
 * not an error (return value 0).  Same fields either way, bit for bit.  enable = 0 switches back.  (No reference counterpart: the
 * reference has no distributed code) */
int rf_comm_enable_direct(rf_plan* plan, int enable, int* enabled);
int rf_comm_direct_enabled(rf_plan* plan, int* enabled);
/* ranks of the plan's communicator as RCCL counts them (ncclCommCount); 0 before rf_comm_init.  What a benchmark line states
 * as "did RCCL see N ranks" (the reference has no distributed code: SURVEY.md section 8e). */
int rf_comm_size(rf_plan* plan, int* nranks);
/* host-side all-reduce of 1 or 2 doubles over the plan's communicator (op 0 = sum, 1 = max), after all
 * queued work of the plan: doubles as a barrier.  With one rank it only synchronises the stream. */
int rf_comm_allreduce_f64(rf_plan* plan, double* inout, int n, int op);

#ifdef __cplusplus
}
#endif
#endif /* RANDOMFIELD_HIP_H */
