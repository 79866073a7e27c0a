"""GPU parity tests (run with ``-m gpu`` on an MI355X).  Everything goes through
the C-ABI (ctypes -> librandomfield_hip.so); the oracle and the golden fixtures
are only the checkers.

Tolerances: float32 fields agree with the reference CPU
path to max|d_gpu - d_cpu| <= 1e-5 * rms(d) on the same noise; in practice the
difference is ~1e-6 * rms (float32 FFT rounding).  k-space cells agree to the
last ulp of log10f (5e-7 relative).  float64 plans: 1e-12.
"""
import os

import numpy as np
import pytest

from conftest import golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPACING = 2.5
TOL_F32 = 1e-5          # * rms, the north-star tolerance
TOL_F64 = 1e-11


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def dpower(default_power):
    return default_power["k"], default_power["Pk"]


def make_plan(hip, shape, dtype, k, Pk, spacing=SPACING):
    from randomfield_amd import powertools
    nx, ny, nz = shape
    plan = hip.DevicePlan(nx, ny, nz, dtype)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, spacing))
    xt, st = cpu_ref.sigma_table(k, Pk, nx, ny, nz, spacing)
    plan.set_power(xt, st)
    return plan


STAGES = ["stages_16x16x16_c64.npz", "stages_32x32x32_c64.npz", "stages_16x32x64_c64.npz",
          "stages_16x16x16_c128.npz", "stages_32x32x32_c128.npz",
          # the reference's own test shapes (tests/test_transform.py:11): non-power-of-two axes, generic kernels
          "stages_4x6x8_c64.npz", "stages_6x4x12_c64.npz", "stages_4x6x8_c128.npz"]


@pytest.mark.parametrize("name", STAGES)
def test_kspace_and_field_against_reference_fixtures(hip, dpower, name):
    """rows K,T,R,S (rf_generate), row X (rf_execute_c2r), fused rf_realise, row D
    (rf_moments) against the reference's own outputs for the same seed."""
    g = golden(name)
    shape = tuple(int(v) for v in g["shape"])
    dtype = g["kspace"].dtype
    tol = TOL_F32 if dtype == np.complex64 else TOL_F64
    rms = float(g["rms"])
    nx, ny, nz = shape
    plan = make_plan(hip, shape, dtype, *dpower)
    noise = cpu_ref.reference_noise(int(g["seed"]), nx * ny * (nz // 2 + 1))

    plan.generate(noise=noise)
    ks = plan.download_k()
    scale = np.max(np.abs(g["kspace"]))
    assert np.max(np.abs(ks - g["kspace"])) <= (5e-7 if dtype == np.complex64 else 1e-14) * scale
    assert ks[0, 0, 0] == 0
    assert np.array_equal(ks.imag == 0, g["kspace"].imag == 0)           # same self-conjugate zeros
    assert cpu_ref.is_hermitian_packed(ks, rtol=0, atol=0)                # exact conjugate pairs

    plan.execute_c2r()
    d1 = plan.download_real()
    assert d1.shape == shape and d1.dtype == g["delta"].dtype
    assert np.max(np.abs(d1 - g["delta"])) <= tol * rms

    # exact reference k-space uploaded -> c2r (row X alone)
    plan.upload_k(g["kspace"])
    plan.execute_c2r()
    assert np.max(np.abs(plan.download_real() - g["delta"])) <= tol * rms

    plan.realise(noise=noise)                                             # fused path
    d2 = plan.download_real()
    assert np.max(np.abs(d2 - g["delta"])) <= tol * rms
    mean, std = plan.moments()
    assert abs(std - rms) <= tol * rms and abs(mean) < 1e-6 * rms
    padded = plan.download_real(padded=True)
    assert padded.shape == (nx, ny, nz + 2) and np.array_equal(padded[:, :, :nz], d2)
    part = plan.download_real(x0=nx // 2, x1=nx // 2 + 2)
    assert np.array_equal(part, d2[nx // 2:nx // 2 + 2])
    plan.close()


@pytest.mark.parametrize("shape", [(2048, 16, 64), (16, 2048, 64), (16, 16, 2048)])
def test_2048_point_axes_against_reference_fixtures(hip, dpower, shape):
    """The longest axis the tiled kernels serve (BASELINE config 4's axis length), pinned to the REFERENCE's own run of
    fill_with_log10k .. Plan.execute at (2048,16,64), (16,2048,64), (16,16,2048) (oracle/make_golden.py, subsampled: a value of
    delta depends on every mode of its line).  Every route through the 2048-point kernels: rows K..S unfused + row X from k space
    (whole-column x pass reading k space, Col2 y pass, 1024-complex z rows), the fused exact-chain realisation, and the drop-in API
    with rng='reference' (MT19937 replay on the device + the fast generation pass, Col2 form at nx = 2048)."""
    from randomfield_amd import Generator
    g = golden("axis2048_%dx%dx%d_c64.npz" % shape)
    assert tuple(int(v) for v in g["shape"]) == shape
    nx, ny, nz = shape
    sd, sk = (tuple(int(v) for v in g[k]) for k in ("stride_delta", "stride_k"))
    rms, kmax = float(g["rms"]), float(g["kspace_absmax"])
    plan = make_plan(hip, shape, np.complex64, *dpower)
    noise = cpu_ref.reference_noise(int(g["seed"]), nx * ny * (nz // 2 + 1))

    def check_field(d, what):
        assert d.shape == shape and d.dtype == np.float32
        assert np.max(np.abs(d[::sd[0], ::sd[1], ::sd[2]] - g["sub"])) <= TOL_F32 * rms, what
        assert np.max(np.abs(d[0, 0, :4] - g["first"])) <= TOL_F32 * rms and np.max(np.abs(d[-1, -1, -4:] - g["last"])) <= TOL_F32 * rms, what
        assert abs(float(d.min()) - float(g["min"])) <= 2 * TOL_F32 * rms and abs(float(d.max()) - float(g["max"])) <= 2 * TOL_F32 * rms, what

    plan.generate(noise=noise)
    ks = plan.download_k()
    assert np.max(np.abs(ks[::sk[0], ::sk[1], ::sk[2]] - g["kspace_sub"])) <= 5e-7 * kmax
    assert ks[0, 0, 0] == 0 and cpu_ref.is_hermitian_packed(ks, rtol=0, atol=0)
    plan.execute_c2r()
    check_field(plan.download_real(), "rf_generate + rf_execute_c2r")
    mean, std = plan.moments()
    assert abs(std - rms) <= TOL_F32 * rms and abs(mean - float(g["mean"])) <= 1e-6 * rms
    plan.realise(noise=noise)
    check_field(plan.download_real(), "rf_realise (exact chain, host deviates)")
    assert abs(plan.moments()[1] - rms) <= TOL_F32 * rms
    plan.close()
    gen = Generator(nx, ny, nz, SPACING)                      # rng='reference' is the default: same seed, same field
    check_field(gen.generate_delta_field(seed=int(g["seed"]), save_potential=False), "Generator(rng='reference')")
    assert abs(float(gen.delta_field_rms) - rms) <= TOL_F32 * rms
    gen.plan_c2r.device.close()


@pytest.mark.parametrize("n,tag", [(64, "c64"), (128, "c64"), (64, "c128"), (128, "c128")])
def test_summary_grids(hip, dpower, n, tag):
    g = golden("summary_%d_%s.npz" % (n, tag))
    dtype = np.complex64 if tag == "c64" else np.complex128
    tol = TOL_F32 if tag == "c64" else TOL_F64
    plan = make_plan(hip, (n, n, n), dtype, *dpower)
    noise = cpu_ref.reference_noise(123, n * n * (n // 2 + 1))
    plan.realise(noise=noise)
    d = plan.download_real()
    rms = float(g["rms"])
    assert np.max(np.abs(d[::8, ::8, ::8] - g["sub"])) <= tol * rms
    assert np.max(np.abs(d[0, 0, :4] - g["first"])) <= tol * rms
    assert np.max(np.abs(d[-1, -1, -4:] - g["last"])) <= tol * rms
    mean, std = plan.moments()
    assert abs(std - rms) <= tol * rms
    assert abs(d.min() - float(g["min"])) <= 2 * tol * rms and abs(d.max() - float(g["max"])) <= 2 * tol * rms
    plan.close()


@pytest.mark.parametrize("shape", [(256, 256, 256), (64, 128, 256), (512, 16, 32), (8, 8, 16), (16, 1024, 64)])
def test_full_field_against_oracle(hip, dpower, shape):
    """Whole-array comparison with the oracle run here on the same noise (sizes the
    oracle finishes in seconds), incl. anisotropic grids and every pass shape."""
    nx, ny, nz = shape
    k, Pk = dpower
    noise = cpu_ref.reference_noise(7, nx * ny * (nz // 2 + 1))
    ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, double_fft=True)
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    plan.realise(noise=noise)
    d = plan.download_real()
    assert np.max(np.abs(d - ref)) <= TOL_F32 * rms
    assert abs(plan.moments()[1] - rms) <= TOL_F32 * rms
    plan.close()


def _check_large_summary(dev, g, check_kspace, TOL_F32=TOL_F32, ktol=5e-6):
    """device field (and k space) against a summary fixture oracle/make_golden_large.py made from the REFERENCE's own run
    (TOL_F32: the field tolerance in units of the rms -- the float64 variant passes its own)"""
    n = int(g["shape"][0])
    s = n // 16
    rms = float(g["rms"])
    mean, std = dev.moments()
    # (the reference's own float32 np.std over 2^30 values carries ~5e-6 relative accumulation error)
    assert abs(std - rms) <= TOL_F32 * rms and abs(mean - float(g["mean"])) <= 1e-6 * rms
    sub = np.stack([dev.download_real(x0=ix, x1=ix + 1)[0, ::s, ::s] for ix in range(0, n, s)])
    assert sub.shape == g["sub"].shape and sub.size == 4096
    assert np.max(np.abs(sub - g["sub"])) <= TOL_F32 * rms
    first = dev.download_real(x0=0, x1=1)[0, 0, :4]
    last = dev.download_real(x0=n - 1, x1=n)[0, -1, -4:]
    assert np.max(np.abs(first - g["first"])) <= TOL_F32 * rms and np.max(np.abs(last - g["last"])) <= TOL_F32 * rms
    lo, hi, sumsq = np.inf, -np.inf, 0.0
    for x0 in range(0, n, 64):
        blk = dev.download_real(x0=x0, x1=x0 + 64)
        lo, hi = min(lo, float(blk.min())), max(hi, float(blk.max()))
        sumsq += float((blk.astype(np.float64) ** 2).sum())
    assert abs(lo - float(g["min"])) <= 2 * TOL_F32 * rms and abs(hi - float(g["max"])) <= 2 * TOL_F32 * rms
    assert abs(sumsq - float(g["sumsq"])) <= 1e-5 * float(g["sumsq"])
    if check_kspace:
        ks = dev.download_k()
        scale = np.abs(g["kspace_sub"]).max()
        assert np.max(np.abs(ks[::s, ::s, 0] - g["plane0_sub"])) <= ktol * scale
        assert np.max(np.abs(ks[::s, ::s, n // 2] - g["nyq_sub"])) <= ktol * scale
        assert np.max(np.abs(ks[::s, ::s, 1::max(1, (n // 2) // 8)] - g["kspace_sub"])) <= ktol * scale


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_baseline_sizes_against_reference_summaries_host_noise(hip, dpower, n):
    """BASELINE configs 1-3 sizes (256^3, 512^3, 1024^3 float32), parity mode: numpy's deviates for seed 123 supplied by the
    host, exact reference dtype chain on the GPU, against tests/golden/summary_<n>_c64.npz -- 4096 field values, the
    SURVEY 8c spot values, rms / mean / min / max / sum of squares, and the two Hermitian planes + 8 more planes of k space
    (subsampled) of the REFERENCE's own run (oracle/make_golden_large.py)."""
    g = golden("summary_%d_c64.npz" % n)
    plan = make_plan(hip, (n, n, n), np.complex64, *dpower)
    noise = cpu_ref.reference_noise(123, n * n * (n // 2 + 1))
    plan.generate(noise=noise)                  # rows K,T,R,S into the API-layout k array
    plan.execute_c2r()                          # row X
    del noise
    _check_large_summary(plan, g, check_kspace=True)
    plan.realise(noise="resident")              # the fused path on the same (resident) deviates
    _check_large_summary(plan, g, check_kspace=False)
    plan.close()


def test_config5_size_float64_against_reference_summary(hip, dpower):
    """BASELINE config 5's grid and dtype (1024^3 complex128 / float64), numpy's deviates for seed 123 from the host, against
    tests/golden/summary_1024_c128.npz (the reference's own complex128 run, 225 s and ~35 GB in the build container)."""
    g = golden("summary_1024_c128.npz")
    n = 1024
    plan = make_plan(hip, (n, n, n), np.complex128, *dpower)
    noise = cpu_ref.reference_noise(123, n * n * (n // 2 + 1))
    plan.generate(noise=noise)
    plan.execute_c2r()
    del noise
    _check_large_summary(plan, g, check_kspace=True, TOL_F32=TOL_F64, ktol=1e-12)
    plan.close()


@pytest.mark.parametrize("n", [512, 1024])
def test_baseline_sizes_generator_reference_rng(hip, n):
    """The same sizes through the Generator API with the default rng='reference': the MT19937 + polar stream of seed 123 is
    replayed on the GPU (no host deviates), and the field must reproduce the reference's summary fixture."""
    from randomfield_amd import Generator
    g = golden("summary_%d_c64.npz" % n)
    gen = Generator(n, n, n, SPACING, backend="hip")
    assert gen.rng == "reference"
    gen.generate_delta_field(seed=123, download=False, save_potential=False)
    assert abs(float(gen.delta_field_rms) - float(g["rms"])) <= TOL_F32 * float(g["rms"])
    dev = gen.plan_c2r.device
    _check_large_summary(dev, g, check_kspace=False)
    dev.close()


def test_native_rng_matches_oracle_restatement(hip, dpower):
    """Native Philox4x32-7 + Box-Muller mode, value by value against the oracle's
    restatement of the same counter-based stream.  The default (fast) generation
    forms sigma and the deviates with float32 hardware log / sin / cos on float32
    AND float64 plans: held to north_star's 1e-5 * rms (measured 4 - 8e-6; rounds 1 - 4 allowed 2e-5 here while the
    bench-instantiation test already held 1e-5).  The exact-chain flavour on a float64 plan
    reproduces the float64 restatement to 1e-11."""
    k, Pk = dpower
    for dtype, tol in ((np.complex64, TOL_F32), (np.complex128, TOL_F64)):
        shape = (64, 32, 128)
        nx, ny, nz = shape
        plan = make_plan(hip, shape, dtype, k, Pk)
        plan.realise(seed=2024)
        d = plan.download_real()
        noise = cpu_ref.native_noise(2024, nx, ny, nz, dtype)
        ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=dtype, double_fft=True)
        assert np.max(np.abs(d - ref)) <= TOL_F32 * rms
        # unfused path (generate -> k-space -> c2r) equals the fused one
        plan.generate(seed=2024)
        ks = plan.download_k()
        kref = cpu_ref.generate_kspace(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=dtype)
        assert np.max(np.abs(ks - kref)) <= tol * np.max(np.abs(kref))
        plan.execute_c2r()
        assert np.max(np.abs(plan.download_real() - d)) <= TOL_F32 * rms
        # the fast float32 generation flavour (default) and the exact-chain flavour agree
        plan.set_exact_generation(True)
        plan.realise(seed=2024)
        assert np.max(np.abs(plan.download_real() - ref)) <= tol * rms
        plan.set_exact_generation(False)
        # deterministic: same seed twice is bitwise identical, another seed is not
        plan.realise(seed=2024)
        assert np.array_equal(plan.download_real(), d)
        plan.realise(seed=2025)
        assert not np.array_equal(plan.download_real(), d)
        plan.close()


def test_native_gaussian_variance(hip):
    """The reference's statistical pin (tests/test_generate.py:24-62) with the native RNG."""
    from scipy.special import erf
    g = golden("variance_64.npz")
    spacing, n = 2.5, 64
    kmin, kmax, sigma = (2 * np.pi) / (spacing * n), np.pi / spacing, 2.5 * spacing
    calc = 1.23 / (2 * np.pi) ** 1.5 / sigma ** 3 * (
        erf(kmax * sigma / np.sqrt(2)) ** 3 - erf(kmin * sigma / np.sqrt(2)) ** 3)
    plan = make_plan(hip, (n, n, n), np.complex64, g["k"], g["Pk"], spacing)
    var = []
    for trial in range(10):
        plan.realise(seed=123 + trial)
        mean, std = plan.moments()
        assert abs(mean) < 1e-6
        var.append(std ** 2)
    assert abs(np.mean(var) - calc) < 0.01 * calc
    plan.close()


def test_large_grid_properties(hip, dpower):
    """BASELINE-size checks through size-independent properties (1024^3 float32):
    zero mean (DC mode is exactly 0), rms equal to the Parseval sum of the sigma
    table over the grid's modes within sampling noise, run-to-run determinism, and
    fused == graph-replayed batch."""
    n = 1024
    k, Pk = dpower
    plan = make_plan(hip, (n, n, n), np.complex64, k, Pk)
    plan.realise(seed=123)
    mean, std = plan.moments()
    slab = plan.download_real(x0=5, x1=6).copy()
    assert abs(mean) < 1e-6 and np.isfinite(slab).all()
    # expected variance: sum over all modes of |delta_k|^2 / N3^2 with <|delta_k|^2> = 2 sigma_k^2 (sigma^2 on
    # the 8 real modes).  Evaluate on a coarse |k| histogram of the grid: the reference run gives 2.3137536.
    assert abs(std - 2.3137) < 5e-3
    assert abs(slab.std() - std) < 0.05 * std
    plan.realise(seed=123)
    assert np.array_equal(plan.download_real(x0=5, x1=6), slab)
    rms = plan.realise_batch([11, 12, 123])
    assert abs(rms[2] - std) <= 1e-12 * std
    assert np.array_equal(plan.download_real(x0=5, x1=6), slab)
    assert abs(rms[0] - 2.3137) < 5e-3 and rms[0] != rms[1]
    plan.close()


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_lognormal_and_scaling(hip, tag):
    """row L: lognormal map with a growth table along z, then per-z scaling."""
    g = golden("lognormal_%s.npz" % tag)
    from randomfield_amd import cosmotools
    delta = g["delta"]
    nx, ny, nz = delta.shape
    dtype = np.complex64 if tag == "f32" else np.complex128
    plan = hip.DevicePlan(nx, ny, nz, dtype)
    plan.upload_real(delta)
    assert np.array_equal(plan.download_real(), delta)
    sigma = g["sigma_vec"][()]
    a_z, b_z = cosmotools.lognormal_tables(g["growth_z"], sigma, nz)
    plan.lognormal(a_z, b_z, float(sigma))
    out = plan.download_real()
    assert np.all(out > 0)
    tol = 2e-6 if tag == "f32" else 1e-14
    assert np.max(np.abs(out - g["out_vec"]) / g["out_vec"]) <= tol
    dens = np.linspace(1.0, 2.0, nz)
    plan.scale_z(dens)
    ref = cpu_ref.scale_z(g["out_vec"].copy(), dens)
    assert np.max(np.abs(plan.download_real() - ref) / ref) <= tol
    plan.affine_z(np.full(nz, 0.5), 1.0)
    ref = ref * 0.5 + 1
    assert np.max(np.abs(plan.download_real() - ref) / ref) <= 2 * tol
    plan.close()


def test_generator_api_hip_backend(hip):
    """The drop-in API: Generator(...).generate_delta_field(seed) on the GPU gives the
    reference's field for the same seed (tests/test_generate.py:16-21 + parity)."""
    from randomfield_amd import Generator
    g = golden("summary_64_c64.npz")
    gen = Generator(64, 64, 64, 2.5)                                  # default backend 'hip', rng 'reference'
    assert gen.backend == "hip" and gen.plan_c2r.device is not None
    data = gen.generate_delta_field(seed=123)                         # default save_potential=True
    assert data.shape == (64, 64, 64) and data.dtype == np.float32
    assert abs(np.mean(data)) < 1e-3
    rms = float(g["rms"])
    assert np.max(np.abs(data[::8, ::8, ::8] - g["sub"])) <= TOL_F32 * rms
    assert abs(gen.delta_field_rms - rms) <= TOL_F32 * rms and isinstance(gen.delta_field_rms, np.float32)
    assert data.base is not None                                      # a view of the plan's buffer
    first = data.copy()
    again = gen.generate_delta_field(seed=123, save_potential=False).copy()  # fused path (float32 sigma arithmetic), same answer
    assert np.max(np.abs(again - first)) <= 3e-6 * rms and gen.potential is None
    assert np.max(np.abs(again[::8, ::8, ::8] - g["sub"])) <= TOL_F32 * rms
    # the device's power tables follow the smoothing length from call to call (they are only re-sent when they change)
    smooth = gen.generate_delta_field(seed=123, smoothing_length_Mpc_h=5.0, save_potential=False).copy()
    assert float(gen.delta_field_rms) < 0.8 * rms and not np.allclose(smooth, first)
    back = gen.generate_delta_field(seed=123, save_potential=False)
    assert np.array_equal(back, again)
    nat = Generator(64, 64, 64, 2.5, rng="native")
    a = nat.generate_delta_field(seed=5, save_potential=False).copy()
    b = nat.generate_delta_field(seed=5, save_potential=False)
    assert np.array_equal(a, b) and abs(nat.delta_field_rms - rms) < 0.05 * rms
    assert nat.generate_delta_field(seed=6, save_potential=False, download=False) is None
    assert not np.array_equal(nat.download_field(), a)


def test_generator_potential_and_density(hip, dpower):
    """save_potential / Newtonian potential / density through the drop-in Generator, against the reference's own
    fixture (potential) and the oracle's restatements (generate.py:200-217, 232-280, 333-343) -- not against this
    repo's numpy backend."""
    from randomfield_amd import Generator
    k, Pk = dpower
    gp = golden("potential_16_c64.npz")
    z = np.linspace(0, 0.1, 16)
    growth, density = np.exp(-z), 1 + z
    gen = Generator(16, 16, 16, 2.5, growth_function=growth, mean_matter_density=density, redshifts=z)
    delta = gen.generate_delta_field(seed=123, save_potential=True).copy()
    pot = gen.potential.download()
    assert np.max(np.abs(pot - gp["potential"])) <= 1e-6 * np.max(np.abs(gp["potential"]))
    dref, rms = cpu_ref.generate_delta_field(16, 16, 16, 2.5, k, Pk, seed=123)
    assert np.max(np.abs(delta - dref)) <= TOL_F32 * rms
    assert abs(float(gen.delta_field_rms) - rms) <= TOL_F32 * rms
    # Newtonian potential: c2r of scale * (reference's saved potential), times G(z) / (1 + z) (generate.py:333-343)
    phi = gen.calculate_newtonian_potential(scale=-1.5)
    phi_ref = np.fft.irfftn(-1.5 * gp["potential"].astype(np.complex128), s=(16, 16, 16), axes=(0, 1, 2)) * (growth / (1 + z))
    assert np.max(np.abs(phi - phi_ref)) <= TOL_F32 * phi_ref.std()
    # density: lognormal map with sigma = rms and the growth function, times the mean matter density (generate.py:268-273)
    gen.generate_delta_field(seed=123, save_potential=False)
    rho = gen.convert_delta_to_density()
    rho_ref = cpu_ref.scale_z(cpu_ref.lognormal(dref.copy(), growth, sigma=dref.dtype.type(rms)), density)
    assert np.all(rho > 0) and np.max(np.abs(rho - rho_ref) / rho_ref) <= 1e-4   # exp() amplifies 1e-6*rms
    gen.generate_delta_field(seed=123, save_potential=False)
    lin = gen.convert_delta_to_density(apply_lognormal_transform=False)
    lin_ref = (dref.astype(np.float64) * growth + 1) * density                     # generate.py:271-273
    assert np.max(np.abs(lin - lin_ref)) <= 1e-5 * np.abs(lin_ref).max()


def test_plan_api_hip_backend(hip):
    """transform.Plan on the hip backend: same host arrays / aliasing, GPU transform."""
    from randomfield_amd.transform import Plan, symmetrize
    rng = np.random.RandomState(3)
    for dtype, tol in ((np.complex64, 2e-6), (np.complex128, 1e-13)):
        plan = Plan(shape=(16, 32, 64), dtype_in=dtype)
        assert plan.backend == "hip"
        n = 2 * plan.data_in.size
        plan.data_in.view(plan.data_out.dtype).reshape(n)[:] = rng.normal(size=n)
        symmetrize(plan.data_in, packed=True)
        ks = plan.data_in.copy()
        out = plan.execute()
        assert out.shape == (16, 32, 64) and (out.base is plan.data_in or out.base is plan.data_in.base)
        ref = np.fft.irfftn(ks.astype(np.complex128), s=(16, 32, 64), axes=(0, 1, 2))
        assert np.max(np.abs(out - ref)) <= tol * ref.std() * 10
        # input whose kz = 0 / nz/2 planes are NOT Hermitian: numpy's irfftn (the reference backend, transform.py:314)
        # still defines an answer, and the packed device layout must give the same one
        plan.data_in.view(plan.data_out.dtype).reshape(n)[:] = rng.normal(size=n)
        ks = plan.data_in.copy()
        out = plan.execute()
        ref = np.fft.irfftn(ks.astype(np.complex128), s=(16, 32, 64), axes=(0, 1, 2))
        assert np.max(np.abs(out - ref)) <= tol * ref.std() * 10


def test_errors_are_loud(hip, dpower):
    with pytest.raises(RuntimeError):
        hip.DevicePlan(4, 6, 7)                                      # unsupported shape (odd axis): no silent CPU path
    with pytest.raises(RuntimeError):
        hip.DevicePlan(16418, 16, 16)                                # 2 x 8209 (prime): neither one line of the LDS nor two factors that fit
    with pytest.raises(RuntimeError):
        hip.DevicePlan(8198, 16, 16, np.complex128)                  # (complex128 lines: up to 4096 points; 8198 = 2 x 4099)
    plan = hip.DevicePlan(16, 16, 16)
    with pytest.raises(RuntimeError):
        plan.realise(seed=1)                                         # tables not set
    with pytest.raises(RuntimeError):
        plan.execute_c2r()                                           # no k-space data
    with pytest.raises(RuntimeError):
        plan.moments()
    with pytest.raises(ValueError):
        plan.realise(noise=np.zeros(10))
    plan.close()
    from randomfield_amd.transform import Plan
    with pytest.raises(RuntimeError):
        Plan(shape=(16418, 16, 16), dtype_in=np.complex64)           # hip backend refuses, does not fall back


def _virtual_rank_field(hip, shape, dtype, k, Pk, nranks, seed=None, noise=None, exact=False):
    """Run the slab pipeline with `nranks` virtual ranks on one device: forward (generation + x + y on the
    kz slab), all-to-all by device copies, backward (z pass on the x slab); returns the assembled field
    and the global (sum, sumsq)."""
    nx, ny, nz = shape
    from randomfield_amd import powertools
    plans = []
    for r in range(nranks):
        p = hip.DevicePlan(nx, ny, nz, dtype, nranks=nranks, rank=r)
        p.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
        p.set_power(*cpu_ref.sigma_table(k, Pk, nx, ny, nz, SPACING))
        p.set_exact_generation(exact)
        plans.append(p)
    for p in plans:
        p.slab_forward(seed=seed or 0, noise=noise)
    hip.DevicePlan.slab_exchange_local(plans)
    parts, s1, s2 = [], 0.0, 0.0
    for p in plans:
        p.slab_backward()
        parts.append(p.download_real())
        a, b = p.slab_stats()
        s1, s2 = s1 + a, s2 + b
    for p in plans:
        p.close()
    return np.concatenate(parts, axis=0), s1, s2


@pytest.mark.parametrize("shape", [(64, 64, 64), (32, 128, 256), (256, 64, 128)])
@pytest.mark.parametrize("nranks", [2, 4, 8])
def test_slab_decomposition_is_rank_count_invariant(hip, dpower, shape, nranks):
    """P = 1 and P = 2, 4, 8 give the same field.  Virtual ranks on one device exercise the kz-slab
    generation, slab x/y passes, the all-to-all block layout and the gathering z pass; only the RCCL
    transport itself is replaced by device copies."""
    nx, ny, nz = shape
    if (nz // 2) % (2 * nranks) or nx % nranks:
        pytest.skip("shape not divisible")
    k, Pk = dpower
    one = make_plan(hip, shape, np.complex64, k, Pk)
    one.realise(seed=77)                                      # native RNG, fast generation flavour
    ref = one.download_real()
    mean, std = one.moments()
    field, s1, s2 = _virtual_rank_field(hip, shape, np.complex64, k, Pk, nranks, seed=77)
    # same cells, same draws; identical up to float32 rounding (different kernel instantiations -- e.g. the
    # split / unsplit kz=0 repair -- may contract multiply-adds differently), 20x below the FFT's own error
    assert np.max(np.abs(field - ref)) <= 1e-6 * std
    n = float(ref.size)
    assert abs(np.sqrt(s2 / n - (s1 / n) ** 2) - std) <= 1e-7 * std
    # external-noise (parity) mode through the exact generation kernel
    noise = cpu_ref.reference_noise(5, nx * ny * (nz // 2 + 1))
    one.realise(noise=noise)
    ref = one.download_real()
    field, s1, s2 = _virtual_rank_field(hip, shape, np.complex64, k, Pk, nranks, noise=noise)
    assert np.max(np.abs(field - ref)) <= 1e-6 * std
    one.close()


def test_slab_float64_and_rccl_single_rank(hip, dpower):
    k, Pk = dpower
    shape = (32, 32, 64)
    one = make_plan(hip, shape, np.complex128, k, Pk)
    one.realise(seed=3)
    ref = one.download_real()
    field, s1, s2 = _virtual_rank_field(hip, shape, np.complex128, k, Pk, 4, seed=3)
    # the default (fast) generation works in float32: kernel instantiations may contract multiply-adds differently
    assert np.max(np.abs(field - ref)) <= 1e-6 * ref.std()
    # with the exact float64 chain the decomposition is invariant to double-precision rounding
    one.set_exact_generation(True)
    one.realise(seed=3)
    ref_exact = one.download_real()
    field, s1, s2 = _virtual_rank_field(hip, shape, np.complex128, k, Pk, 4, seed=3, exact=True)
    assert np.max(np.abs(field - ref_exact)) <= 1e-13 * ref_exact.std()
    one.set_exact_generation(False)
    # nx = 1024: the float64 generation pass as two 512-point transforms per tile (Col2), whole grid and on kz slabs
    big = make_plan(hip, (1024, 8, 128), np.complex128, k, Pk)
    big.realise(seed=3)
    bref = big.download_real()
    big.close()
    field, s1, s2 = _virtual_rank_field(hip, (1024, 8, 128), np.complex128, k, Pk, 4, seed=3)
    assert np.max(np.abs(field - bref)) <= 1e-6 * bref.std()
    # the RCCL library loads, a communicator initialises and a collective runs (1 rank: all a 1-GPU box allows)
    import sys
    if "torch" in sys.modules:
        pytest.skip("PyTorch's bundled ROCm runtime is loaded in this process; RCCL is exercised torch-free")
    uid = hip.DevicePlan.comm_unique_id()
    assert len(uid) == 128
    one.comm_init(uid)
    assert one.allreduce([2.5, -1.0], op="max").tolist() == [2.5, -1.0]
    one.barrier()
    one.realise(seed=3)
    assert np.array_equal(one.download_real(), ref)
    # the shared replay's collective calls on that communicator (integer all-reduce of the counts, own-block copy): one rank
    # holds every segment, and the deviates must be those of the plain replay
    one.reference_noise(77)
    want = one.download_noise()
    assert one.reference_noise_shared(77) >= 32 * 32 * 33
    assert np.array_equal(one.download_noise(), want)
    one.close()


@pytest.mark.parametrize("shape", [(8, 8, 16), (16, 32, 64), (64, 64, 64), (32, 128, 256), (256, 16, 1024)])
def test_forward_r2c_against_numpy(hip, shape):
    """rf_execute_r2c (transform.py:199-206,270): forward, unnormalised, API k layout; and c2r(r2c(x)) = x."""
    rng = np.random.RandomState(9)
    for dtype, ct, tol in ((np.float32, np.complex64, 3e-6), (np.float64, np.complex128, 1e-13)):
        nx, ny, nz = shape
        f = rng.normal(size=shape).astype(dtype)
        plan = hip.DevicePlan(nx, ny, nz, ct)
        plan.upload_real(f)
        plan.execute_r2c()
        spec = plan.download_k()
        ref = np.fft.rfftn(f.astype(np.float64), axes=(0, 1, 2))
        assert spec.shape == (nx, ny, nz // 2 + 1) and spec.dtype == ct
        assert np.max(np.abs(spec - ref)) <= tol * np.sqrt(f.size) * 3
        assert cpu_ref.is_hermitian_packed(spec, rtol=0, atol=tol * np.sqrt(f.size) * 3)
        plan.execute_c2r()                                              # k buffer -> real field
        assert np.max(np.abs(plan.download_real() - f)) <= 10 * tol
        plan.close()
    g = golden("r2c_8x16x32_f32.npz")
    plan = hip.DevicePlan(8, 16, 32, np.complex64)
    plan.upload_real(g["field"])
    plan.execute_r2c()
    assert np.allclose(plan.download_k(), g["spectrum"], rtol=0, atol=1e-4)       # the reference's own rfftn output
    plan.close()


def test_round_trip_at_full_size(hip, dpower):
    """Size-independent property at BASELINE size: r2c(c2r(K)) reproduces the generated k space and
    c2r(r2c(delta)) the field (1024^3 float32, values compared on slabs / planes)."""
    n = 1024
    k, Pk = dpower
    plan = make_plan(hip, (n, n, n), np.complex64, k, Pk)
    plan.realise(seed=5)
    mean, std = plan.moments()
    slab = plan.download_real(x0=100, x1=101).copy()
    plan.execute_r2c()                                                   # delta(x) -> delta(k)
    plan.execute_c2r()                                                   # and back
    back = plan.download_real(x0=100, x1=101)
    assert np.max(np.abs(back - slab)) <= 2e-5 * std
    m2, s2 = plan.moments()
    assert abs(s2 - std) <= 1e-5 * std
    plan.close()


def test_plan_r2c_and_reverse_on_device(hip):
    """transform.Plan forward plans and create_reverse_plan on the hip backend (tests/test_transform.py:270-298)."""
    from randomfield_amd.transform import Plan
    rng = np.random.RandomState(4)
    shape = (16, 16, 32)
    for ftype in (np.float32, np.float64):
        for overwrite in (True, False):
            plan_f = Plan(shape=shape, dtype_in=ftype, inverse=False, packed=True, overwrite=overwrite)
            assert plan_f.backend == "hip"
            plan_r = plan_f.create_reverse_plan(reuse_output=True, overwrite=True)
            assert plan_r.device is plan_f.device and plan_r.nbytes_allocated == 0
            plan_f.data_in[:] = rng.normal(size=shape)
            original = np.copy(plan_f.data_in)
            spec = plan_f.execute()
            assert np.allclose(spec, np.fft.rfftn(original.astype(np.float64), axes=(0, 1, 2)), rtol=0,
                               atol=2e-4 if ftype == np.float32 else 1e-10)
            result = plan_r.execute()
            assert np.allclose(original, result, atol=1e-5 if ftype == np.float32 else 1e-12)


@pytest.mark.parametrize("shape", [(64, 64, 64), (128, 32, 256)])
def test_pipelined_slab_batch_matches_plain_path(hip, dpower, shape):
    """The multi-GPU code path (slab y pass, exchange, gathering z pass) and its software-pipelined batch
    (two streams, two buffer pairs, events) run on ONE rank (the exchange degenerates to a copy of the own
    block): every realisation's rms and the resident final field must equal the plain single-GPU path."""
    k, Pk = dpower
    seeds = [3, 4, 5, 6, 7]
    plain = make_plan(hip, shape, np.complex64, k, Pk)
    rms_ref = plain.realise_batch(seeds)
    last_ref = plain.download_real()
    slab = make_plan(hip, shape, np.complex64, k, Pk)
    slab.set_force_slab_path(True)
    slab.realise(seed=seeds[-1])
    std = plain.moments()[1]
    assert np.max(np.abs(slab.download_real() - last_ref)) <= 1e-6 * std
    assert abs(slab.moments()[1] - std) <= 1e-7 * std
    for n in (1, 2, 5):                                          # odd and even counts end in different buffers
        rms = slab.realise_batch(seeds[:n])
        assert np.allclose(rms, rms_ref[:n], rtol=1e-7, atol=0)
        plain.realise(seed=seeds[n - 1])
        assert np.max(np.abs(slab.download_real() - plain.download_real())) <= 1e-6 * std
        assert abs(slab.moments()[1] - rms_ref[n - 1]) <= 1e-7 * std
    rms2 = slab.realise_batch(seeds)                              # buffers / events are reusable
    assert np.allclose(rms2, rms_ref, rtol=1e-7, atol=0)
    slab.close()
    plain.close()


def test_exchange_standin_runs_the_real_schedule_on_a_virtual_rank(hip, dpower):
    """rf_slab_set_exchange_standin (diagnostics, bench.py's config-4 entry): a rank of a multi-rank plan WITHOUT a communicator runs
    the multi-GPU schedule -- forward half, exchange on the exchange stream, gathering z pass, pipelined batches -- with a copy kernel
    in the all-to-all's place.  The received segments are the rank's own data for other x slabs, so the result is not a field; what
    is checked: it runs to completion for every width, the moments are finite and reproducible, the own block (segment `rank`) really
    is the forward half's block, and the call is refused where it has no business (single-rank plans, bad widths; a rank without
    communicator and without stand-in still fails loudly)."""
    k, Pk = dpower
    shape, P = (256, 64, 256), 4
    plans = _slab_plans(hip, shape, np.complex64, k, Pk, P)
    p = plans[1]
    with pytest.raises(RuntimeError):
        p.realise(seed=3)                                         # no communicator, no stand-in: loud
    with pytest.raises(RuntimeError):
        p.set_exchange_standin(-1)
    for w in (1, 16, 300):
        p.set_exchange_standin(w)
        p.realise(seed=3)
        m1 = p.moments()
        rms = p.realise_batch([3, 4, 5])
        p.realise(seed=3)
        assert np.isfinite(m1[1]) and m1[1] > 0 and p.moments() == m1 and np.all(np.isfinite(rms)) and len(rms) == 3
    # the same rank through the separate steps with a real (virtual-rank) exchange gives a field; the stand-in run is not one
    p.set_exchange_standin(0)
    with pytest.raises(RuntimeError):
        p.realise(seed=3)
    one = make_plan(hip, shape, np.complex64, k, Pk)
    with pytest.raises(RuntimeError):
        one.set_exchange_standin(16)                              # a single-rank plan exchanges nothing
    one.close()
    for q in plans:
        q.close()


@pytest.mark.parametrize("shape,seed", [((16, 16, 16), 123), ((64, 64, 64), 123), ((128, 128, 256), 7), ((256, 256, 256), 2024)])
def test_mt19937_replay_matches_numpy(hip, dpower, shape, seed):
    """On-GPU replay of np.random.RandomState(seed).normal(size=2*M) (random.py:24-28): MT19937 with jump-ahead
    by t^J mod phi(t), polar rejection with count / scan / fill.  The integer stream is exact; the deviates are
    bit-identical except where the device's double log()/sqrt() round differently from libm's (about 1 %
    of the values, at most 2 ulp): <= 1e-15 relative.  (r2 itself must round like numpy's C code -- two
    products and a sum, no FMA -- or cells with r2 near 1 amplify a 1-ulp difference to ~1e-9.)"""
    nx, ny, nz = shape
    k, Pk = dpower
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    accepted = plan.reference_noise(seed)
    ncells = nx * ny * (nz // 2 + 1)
    assert accepted >= ncells
    got = plan.download_noise()
    ref = cpu_ref.reference_noise(seed, ncells)
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)) <= 1e-15
    assert np.mean(got == ref) > 0.95                                   # mostly bit-identical
    # and the field generated from it is the reference's field for that seed
    plan.realise(noise="resident")
    d = plan.download_real()
    dref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, seed=seed)
    assert np.max(np.abs(d - dref)) <= TOL_F32 * rms
    plan.close()


@pytest.mark.parametrize("shape", [(8, 8, 8), (16, 64, 32), (64, 64, 64), (256, 16, 1024), (32, 128, 256), (8, 16, 2048)])
def test_unpacked_c2c_plan_against_numpy(hip, shape):
    """transform.Plan(packed=False) on the GPU (transform.py:207-213,266-270; the reference's
    tests/test_transform.py round trips): forward = np.fft.fftn, inverse = np.fft.ifftn, in place,
    and a reverse plan that shares the buffer undoes the transform."""
    from randomfield_amd import transform
    rng = np.random.RandomState(3)
    for ct, tol in ((np.complex64, 2e-6), (np.complex128, 1e-14)):
        a = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(ct)
        plan = transform.Plan(shape, dtype_in=ct, inverse=False, packed=False, backend="hip")
        assert plan.device is not None and plan.data_out is plan.data_in
        plan.data_in[:] = a
        out = plan.execute()
        assert out is plan.data_out and out.dtype == ct and out.shape == shape
        ref = np.fft.fftn(a.astype(np.complex128))
        assert np.max(np.abs(out - ref)) <= tol * np.sqrt(a.size) * 4
        back = plan.create_reverse_plan()                  # shares the host buffer and the device plan
        assert back.device is plan.device and back.data_in is plan.data_out
        res = back.execute()
        assert np.max(np.abs(res - a)) <= 20 * tol
        inv = transform.Plan(shape, dtype_in=ct, inverse=True, packed=False, backend="hip")
        inv.data_in[:] = a
        assert np.max(np.abs(inv.execute() - np.fft.ifftn(a.astype(np.complex128)))) <= 4 * tol
        plan.device.close()
        inv.device.close()
    small = transform.Plan((6, 8, 8), dtype_in=np.complex64, packed=False, backend="hip")   # not a power of two: generic kernels
    small.data_in[:] = rng.normal(size=(6, 8, 8))
    src = small.data_in.copy()
    assert np.max(np.abs(small.execute() - np.fft.ifftn(src.astype(np.complex128)))) <= 1e-6
    with pytest.raises(RuntimeError):
        transform.Plan((8, 8, 16418), dtype_in=np.complex64, packed=False, backend="hip")   # nz = 2 x 8209 (prime): beyond every kernel
    with pytest.raises(RuntimeError):
        transform.Plan((8, 8, 8198), dtype_in=np.complex128, packed=False, backend="hip")   # (complex128 lines hold 4096 points; 8198 = 2 x 4099)


@pytest.mark.parametrize("shape", [(8, 8, 16), (16, 8, 64), (8, 16, 256), (4 * 2, 8, 2048), (8, 8, 512), (8, 8, 1024)])
def test_lensing_potential_kernel_against_oracle(hip, shape):
    """rf_lensing_potential (generate.py:352-416 as one prefix scan per row) against the oracle's restatement of
    the reference's slice loop + scipy.integrate.simps(even='avg'), float32 and float64, flat and curved."""
    nx, ny, nz = shape
    rng = np.random.RandomState(5)
    spacing = 2.5
    DC = np.arange(nz) * spacing
    DA = DC * (1 + 0.02 * np.arange(nz) / nz)
    for dtype, ct, tol in ((np.float32, np.complex64, 2e-6), (np.float64, np.complex128, 1e-12)):
        phi = rng.normal(size=shape).astype(dtype)
        plan = hip.DevicePlan(nx, ny, nz, ct)
        plan.upload_real(phi)
        for K, i_min in ((0.0, nz // 32), (0.0, 0), (-3e-8, 3), (2e-8, nz - 2)):
            cot = cpu_ref.cot_k(DC, DA, K)
            plan.lensing_potential(cot, spacing, i_min)
            psi = plan.download_aux()
            ref = cpu_ref.lensing_potential(phi, DC, DA, K=K, i_min=i_min)
            assert psi.dtype == dtype and psi.shape == shape
            assert np.max(np.abs(psi - ref)) <= tol * np.max(np.abs(ref)) + 1e-300
            assert np.array_equal(plan.download_real(), phi)               # the input field is untouched
        plan.close()


@pytest.mark.parametrize("ct", [np.complex64, np.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("nz", [6, 22, 130, 258, 300, 1000])
def test_lensing_potential_kernel_on_generic_row_lengths(hip, nz, ct):
    """lensing_kernel's guarded scalar route: rows that are no whole number of 64-lane segments (256 float32 / 128 float64
    samples) -- shorter than one, one or several and a partial one, and rows of nz = 2 (mod 4) samples, whose starts are not
    16-byte aligned -- flat and curved, with i_min at the row's start, inside the first segment, inside the second where
    the row has two, and on the last two samples.  Against the oracle at the tolerances of the test above."""
    shape = (6, 10, nz)
    dtype, tol = (np.float32, 2e-6) if ct == np.complex64 else (np.float64, 1e-12)
    seg = 64 * (16 // np.dtype(dtype).itemsize)
    spacing = 2.5
    DC = np.arange(nz) * spacing
    DA = DC * (1 + 0.02 * np.arange(nz) / nz)
    i_mins = {0, 3, nz - 2, nz - 1}
    if nz > seg:
        inside_second = seg + min(5, nz - seg - 1)
        assert seg <= inside_second < min(nz, 2 * seg)
        i_mins.add(inside_second)
    phi = np.random.RandomState(nz).normal(size=shape).astype(dtype)
    plan = hip.DevicePlan(*shape, ct)
    assert nz % seg != 0 and not plan.tiled
    plan.upload_real(phi)
    for K in (0.0, -3e-8, 2e-8):
        cot = cpu_ref.cot_k(DC, DA, K)
        for i_min in sorted(i_mins):
            plan.lensing_potential(cot, spacing, i_min)
            psi = plan.download_aux()
            ref = cpu_ref.lensing_potential(phi, DC, DA, K=K, i_min=i_min)
            assert psi.dtype == dtype and psi.shape == shape
            err, scale = float(np.max(np.abs(psi - ref))), float(np.max(np.abs(ref)))
            print("lensing %s %s K = %g, i_min = %d: measured / bound = %.3g" % (shape, dtype.__name__, K, i_min, err / (tol * scale + 1e-300)))
            assert err <= tol * scale + 1e-300, (K, i_min)
            assert np.array_equal(plan.download_real(), phi)               # the input field is untouched
    plan.close()


def test_generator_lensing_potential(hip):
    """The drop-in sequence generate_delta_field(save_potential=True) -> calculate_newtonian_potential ->
    calculate_lensing_potential on the GPU against the oracle applied to the downloaded Newtonian potential."""
    from randomfield_amd import Generator
    nx, ny, nz, spacing = 32, 16, 128, 2.5
    z = np.linspace(0, 0.1, nz)
    DA = np.arange(nz) * spacing * (1 - 0.05 * np.arange(nz) / nz)
    gen = Generator(nx, ny, nz, spacing, backend="hip", growth_function=np.exp(-z), redshifts=z,
                    transverse_distance=DA, curvature_K=-1e-8)
    gen.generate_delta_field(seed=4, save_potential=True)
    phi = gen.calculate_newtonian_potential(scale=-2.5e-5).copy()
    psi = gen.calculate_lensing_potential()
    ref = cpu_ref.lensing_potential(phi, gen.DC, DA, K=-1e-8)
    assert psi.shape == phi.shape and psi.dtype == np.float32
    assert np.max(np.abs(psi - ref)) <= 2e-6 * np.max(np.abs(ref))
    with pytest.raises(ValueError):
        gen.calculate_lensing_potential(i_min=-1)
    gen.plan_c2r.device.close()


def test_randomised_call_sequences(hip, monkeypatch):
    """A few seconds of tools/fuzz_api.py: random shapes, dtypes and call sequences through the C-ABI (realise with
    native / external / replayed noise, generate + c2r, r2c round trips, lognormal, affine, potential, graph batches,
    lensing), every result checked against the oracle or numpy."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_api.py")
    spec = importlib.util.spec_from_file_location("fuzz_api", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr("sys.argv", ["fuzz_api.py", "6", "42"])
    mod.main()


@pytest.mark.parametrize("shape,dtype", [((64, 64, 64), np.complex64), ((256, 64, 128), np.complex64), ((64, 128, 256), np.complex128)])
@pytest.mark.parametrize("nranks", [2, 4, 8])
def test_replicated_generation_mode_matches_single_rank(hip, dpower, shape, dtype, nranks):
    """RF_FLAG_REPLICATED_GENERATION: every (virtual) rank generates all of k space, keeps only its x slab after the
    x pass and finishes locally -- no exchange.  The assembled slabs equal the single-rank field, single realisations
    and batches, and the partial moments add up."""
    nx, ny, nz = shape
    k, Pk = dpower
    one = make_plan(hip, shape, dtype, k, Pk)
    one.realise(seed=77)
    ref = one.download_real()
    mean, std = one.moments()
    parts, s1, s2 = [], 0.0, 0.0
    for r in range(nranks):
        p = hip.DevicePlan(nx, ny, nz, dtype, nranks=nranks, rank=r)
        from randomfield_amd import powertools
        p.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
        p.set_power(*cpu_ref.sigma_table(k, Pk, nx, ny, nz, SPACING))
        p.set_replicated_generation(True)
        p.realise(seed=77)
        part = p.download_real()
        assert part.shape == (nx // nranks, ny, nz)
        a, b = p.slab_stats()
        s1, s2 = s1 + a, s2 + b
        p.realise_batch(np.array([5, 77], dtype=np.uint64), want_rms=False)      # batch path, last seed = 77
        assert np.array_equal(p.download_real(), part)
        parts.append(part)
        with pytest.raises(RuntimeError):
            p.realise(noise=cpu_ref.reference_noise(1, nx * ny * (nz // 2 + 1)))   # needs the native generator
        p.close()
    field = np.concatenate(parts, axis=0)
    assert np.max(np.abs(field - ref)) <= 1e-6 * std
    n = float(nx) * ny * nz
    assert abs(np.sqrt(s2 / n - (s1 / n) ** 2) - std) <= 1e-9 * std
    one.close()


def test_batch_graphs_follow_table_changes(hip, dpower):
    """Captured batch graphs carry the generation tables by value: replacing P(k) (or the k grid) between two batches
    of the same length must not replay the old tables (regression: the graphs used to survive rf_set_power)."""
    k, Pk = dpower
    shape = (64, 64, 64)
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    seeds = np.array([3, 4, 5], dtype=np.uint64)
    rms1 = plan.realise_batch(seeds)
    f1 = plan.download_real()
    xt, st = cpu_ref.sigma_table(k, 4.0 * Pk, 64, 64, 64, SPACING)      # 4 x the power = 2 x the amplitude
    plan.set_power(xt, st)
    rms2 = plan.realise_batch(seeds)
    f2 = plan.download_real()
    assert np.allclose(rms2, 2.0 * rms1, rtol=1e-5)
    assert np.max(np.abs(f2 - 2.0 * f1)) <= 1e-5 * rms2[-1]
    # a different table shape (fewer rows: new record layout) as well
    sub = slice(None, None, 3)
    k3, P3 = np.append(k[sub], k[-1]), np.append(Pk[sub], Pk[-1])
    plan.set_power(*cpu_ref.sigma_table(k3, P3, 64, 64, 64, SPACING))
    rms3 = plan.realise_batch(seeds)
    plan.realise(seed=5)
    assert abs(plan.moments()[1] - rms3[-1]) <= 1e-12 * rms3[-1]
    plan.close()


@pytest.mark.parametrize("shape", [(2048, 8, 32), (8, 2048, 32), (16, 8, 2048)])
def test_float64_plans_with_a_2048_axis(hip, dpower, shape):
    """float64 plans whose length-2048 tile fills a CU's LDS (no room for the fast generation tables: the exact kernel
    is used for nx = 2048) -- regression: such plans failed at creation."""
    nx, ny, nz = shape
    k, Pk = dpower
    plan = make_plan(hip, shape, np.complex128, k, Pk)
    plan.realise(seed=9)
    d = plan.download_real()
    noise = cpu_ref.native_noise(9, nx, ny, nz, np.complex128)
    ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=np.complex128)
    assert np.max(np.abs(d - ref)) <= 2e-5 * rms
    plan.close()


# ---- round 2: the kernel instantiations that bench.py and BASELINE configs 1-5 actually run ----------------
# (nx decides the generation kernel: 512 -> radix 8.8.8 / 16-column tiles, 1024 -> 8.16.8 / 8 columns, 2048 ->
# 8.16.16 / 1024 threads; nz/2 wider than one tile makes the launcher split the pass into the kz = 0 repair launch
# and the `skip_period` main launch, exactly as at 1024^3.)
@pytest.mark.parametrize("shape,dtype", [((1024, 8, 32), np.complex64), ((512, 16, 64), np.complex64),
                                         ((2048, 8, 32), np.complex64), ((1024, 8, 16), np.complex128),
                                         ((1024, 16, 64), np.complex64)])
def test_native_generation_bench_instantiations_against_oracle(hip, dpower, shape, dtype):
    """Native Philox + Box-Muller mode, fast float32 generation, value by value against the oracle's float64
    restatement of the same counter-based stream (generate.py:191-199,218-219 semantics).

    Tolerance: this is the repo's own stream, so no reference parity is claimed for it; the fast flavour forms
    sigma and the deviates with hardware v_log / v_sqrt / v_sin / v_cos in float32.  Measured on MI355X the field
    differs from the float64 restatement by 4-8e-6 * rms (maximum over all cells); the bound asserted is the
    north-star 1e-5 * rms, and the exact-chain flavour (same stream, reference dtype chain) is held to it as well."""
    k, Pk = dpower
    nx, ny, nz = shape
    plan = make_plan(hip, shape, dtype, k, Pk)
    plan.realise(seed=31337)
    d = plan.download_real()
    mean, std = plan.moments()
    noise = cpu_ref.native_noise(31337, nx, ny, nz, dtype)
    ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=dtype, double_fft=True)
    err = float(np.max(np.abs(d - ref)) / rms)
    assert err <= 1e-5, "fast native generation differs from the oracle restatement by %.3g * rms" % err
    assert abs(std - rms) <= 2e-6 * rms
    # graph-replayed batch == eager, and the exact-chain flavour of the same stream
    rms_b = plan.realise_batch([1, 31337])
    assert abs(rms_b[1] - std) <= 1e-12 * std and np.array_equal(plan.download_real(), d)
    plan.set_exact_generation(True)
    plan.realise(seed=31337)
    assert np.max(np.abs(plan.download_real() - ref)) <= (1e-5 if dtype == np.complex64 else TOL_F64) * rms
    plan.close()


def test_config4_shapes_with_virtual_ranks(hip, dpower):
    """BASELINE config 4 at full size: 2048^3 float32 over 8 slabs.  Eight virtual ranks on one MI355X run the
    kernels and layouts of the 8-GPU job (kz-slab generation + x + y, block exchange by device copies, gathering z
    pass); a few x-planes of every slab and the global rms must equal the single-rank 2048^3 field.  ~105 GB of HBM."""
    from randomfield_amd import powertools
    n, P = 2048, 8
    k, Pk = dpower
    try:
        one = make_plan(hip, (n, n, n), np.complex64, k, Pk)
    except RuntimeError as e:          # a smaller card: not the configuration under test
        pytest.skip("2048^3 does not fit this device: %s" % e)
    one.realise(seed=4)
    mean, std = one.moments()
    planes = [0, 255, 256, 1000, 1791, 2047]
    ref = {x: one.download_real(x0=x, x1=x + 1).copy() for x in planes}
    one.close()
    assert abs(mean) < 1e-6 and 1.0 < std < 10.0
    plans = []
    for r in range(P):
        p = hip.DevicePlan(n, n, n, np.complex64, nranks=P, rank=r)
        p.set_kgrid(*powertools.ksq_axes(n, n, n, SPACING))
        p.set_power(*cpu_ref.sigma_table(k, Pk, n, n, n, SPACING))
        plans.append(p)
    for p in plans:
        p.slab_forward(seed=4)
    hip.DevicePlan.slab_exchange_local(plans)
    s1 = s2 = 0.0
    nxl = n // P
    for r, p in enumerate(plans):
        p.slab_backward()
        a, b = p.slab_stats()
        s1, s2 = s1 + a, s2 + b
        for x in planes:
            if r * nxl <= x < (r + 1) * nxl:
                got = p.download_real(x0=x - r * nxl, x1=x - r * nxl + 1)
                assert np.max(np.abs(got - ref[x])) <= 1e-6 * std, "plane %d of rank %d" % (x, r)
    cells = float(n) ** 3
    assert abs(np.sqrt(s2 / cells - (s1 / cells) ** 2) - std) <= 1e-7 * std
    # the same job with the exchange in 4 sub-slabs per rank (RF_FLAG_EXCHANGE_CHUNKS: what a single generate_delta_field call of
    # Generator(distributed=True) overlaps with its own forward half): 32-plane sub-slabs generated, transformed and handed over one
    # by one, 32 segments of 256 B per row in the gathering z pass -- the same cells, the same arithmetic: not one bit differs
    unchunked = {(r, x): p.download_real(x0=x - r * nxl, x1=x - r * nxl + 1).copy() for r, p in enumerate(plans) for x in planes
                 if r * nxl <= x < (r + 1) * nxl}
    for p in plans:
        p.set_exchange_chunks(4)
    for p in plans:
        p.slab_forward(seed=4)
    hip.DevicePlan.slab_exchange_local(plans)
    for r, p in enumerate(plans):
        p.slab_backward()
        for x in planes:
            if r * nxl <= x < (r + 1) * nxl:
                assert np.array_equal(p.download_real(x0=x - r * nxl, x1=x - r * nxl + 1), unchunked[(r, x)]), "plane %d of rank %d, chunked" % (x, r)
    # ... and with the DIRECT exchange (rf_slab_link_direct): every rank's y pass stores its 2048-point tiles straight into the receive
    # buffers of the eight x-slab owners, nothing is copied afterwards -- whole slabs, then 4 sub-slabs: not one bit differs
    for chunks in (1, 4):
        hip.DevicePlan.slab_link_direct(plans, False)
        for p in plans:
            p.set_exchange_chunks(chunks)
        hip.DevicePlan.slab_link_direct(plans)
        for p in plans:
            p.slab_forward(seed=4)
        for r, p in enumerate(plans):
            p.slab_backward()
            for x in planes:
                if r * nxl <= x < (r + 1) * nxl:
                    assert np.array_equal(p.download_real(x0=x - r * nxl, x1=x - r * nxl + 1), unchunked[(r, x)]), "plane %d of rank %d, direct, %d sub-slabs" % (x, r, chunks)
    for p in plans:
        p.close()


@pytest.mark.parametrize("shape,dtype,nranks,chunks", [((64, 32, 128), np.complex64, 2, 2), ((64, 32, 128), np.complex64, 4, 2), ((32, 64, 256), np.complex64, 2, 8),
                                                       ((32, 16, 128), np.complex128, 2, 4), ((1024, 16, 256), np.complex64, 4, 2), ((2048, 8, 256), np.complex64, 2, 4)])
def test_exchange_in_chunks_is_bit_identical(hip, dpower, shape, dtype, nranks, chunks):
    """RF_FLAG_EXCHANGE_CHUNKS: a rank's kz slab generated, x / y-transformed and exchanged as `chunks` sub-slabs (layout
    W = [chunk][nx][ny][nzl / chunks], R = [source][chunk][...]) gives the unchunked slab pipeline's field -- native
    generator, host deviates through the exact chain, uploaded k space and the fused potential store -- and the reverse (r2c)
    exchange keeps its own block layout."""
    k, Pk = dpower
    nx, ny, nz = shape
    plans = _slab_plans(hip, shape, dtype, k, Pk, nranks)
    noise = cpu_ref.reference_noise(5, nx * ny * (nz // 2 + 1))
    want = {}
    for C in (1, chunks):
        for p in plans:
            p.set_exchange_chunks(C)
        got = {"native": _slab_run(hip, plans, seed=11), "host noise": _slab_run(hip, plans, noise=noise),
               "potential": _slab_run(hip, plans, seed=11, source="potential")}
        for p in plans:
            p.generate(seed=12)
        got["k space"] = _slab_run(hip, plans, source="kspace")
        # forward transform of the field just made: rows, reverse exchange (block layout whatever the flag says), columns
        for p in plans:
            p.slab_r2c_rows()
        hip.DevicePlan.slab_exchange_local_reverse(plans)
        for p in plans:
            p.slab_r2c_cols()
        got["r2c"] = _slab_side_array(plans, lambda p: p.download_k(), nz // 2)
        if C == 1:
            want = got
        else:
            # the same cells through the same arithmetic; bit for bit wherever the same kernel instantiations run (sub-slabs
            # narrower than an x-pass tile take the kernel that repairs kz = 0 in every tile: float32 rounding apart)
            for key in want:
                scale = np.abs(want[key]).max() if key == "r2c" else want[key].std()
                assert np.max(np.abs(got[key] - want[key])) <= (2e-6 if dtype == np.complex64 else 1e-13) * scale, (key, C)
            if shape[0] >= 1024:
                assert np.array_equal(got["native"], want["native"]) and np.array_equal(got["k space"], want["k space"])
    with pytest.raises(RuntimeError):
        plans[0].set_exchange_chunks(3)                      # not a power of two
    with pytest.raises(RuntimeError):
        plans[0].set_exchange_chunks(1024)                   # sub-slabs thinner than a tile
    for p in plans:
        p.close()


def test_one_realisation_overlaps_its_own_exchange(hip, dpower):
    """The single-call path of a plan that exchanges in chunks (queue_c2r: forward half of sub-slab c on the plan's stream, its
    exchange on the second stream behind an event, the z pass behind the last exchange) on ONE rank through the forced slab
    path: field and moments of rf_realise, rf_realise_potential + the Newtonian potential, and the pipelined batch equal the
    plain single-GPU plan's."""
    k, Pk = dpower
    shape = (256, 128, 256)
    plain = make_plan(hip, shape, np.complex64, k, Pk)
    slab = make_plan(hip, shape, np.complex64, k, Pk)
    slab.set_force_slab_path(True)
    slab.set_exchange_chunks(4)
    for seed in (3, 4):                                      # (the second call reuses events and buffers)
        plain.realise(seed=seed)
        slab.realise(seed=seed)
        std = plain.moments()[1]
        assert np.max(np.abs(slab.download_real() - plain.download_real())) <= 1e-6 * std
        assert abs(slab.moments()[1] - std) <= 1e-6 * std
        assert len(slab.kernel_ms()) == 5
    plain.realise_potential(seed=9)
    slab.realise_potential(seed=9)
    assert np.max(np.abs(slab.download_real() - plain.download_real())) <= 1e-6 * std
    plain.load_potential(-1.5)
    slab.load_potential(-1.5)
    plain.execute_c2r()
    slab.execute_c2r()
    a, b = plain.download_real(), slab.download_real()
    assert np.max(np.abs(a - b)) <= 2e-6 * a.std()
    rms_ref = plain.realise_batch([5, 6, 7])
    assert np.allclose(slab.realise_batch([5, 6, 7]), rms_ref, rtol=1e-6, atol=0)
    assert np.max(np.abs(slab.download_real() - plain.download_real())) <= 1e-6 * std
    slab.set_exchange_chunks(1)                              # and back
    slab.realise(seed=3)
    plain.realise(seed=3)
    assert np.max(np.abs(slab.download_real() - plain.download_real())) <= 1e-6 * std
    slab.close()
    plain.close()


def test_collectives_leave_the_moments_alone(hip, dpower):
    """A 64-realisation batch on the multi-GPU code path fills every (sum, sumsq) slot the plan starts with; the host
    all-reduces that follow (barrier(), allreduce()) must not use any of them as scratch (round-1 bug)."""
    import sys
    if "torch" in sys.modules:
        pytest.skip("PyTorch's bundled ROCm runtime is loaded in this process; RCCL is exercised torch-free")
    k, Pk = dpower
    plan = make_plan(hip, (32, 32, 64), np.complex64, k, Pk)
    plan.set_force_slab_path(True)
    plan.comm_init(hip.DevicePlan.comm_unique_id())          # one-rank communicator: the collectives really run
    seeds = np.arange(500, 564, dtype=np.uint64)
    rms = plan.realise_batch(seeds)
    plan.barrier()
    assert plan.allreduce([1.5, 2.5]).tolist() == [1.5, 2.5]
    assert abs(plan.moments()[1] - rms[-1]) <= 1e-12 * rms[-1]
    rms2 = plan.realise_batch(seeds)
    assert np.array_equal(rms, rms2)
    plan.close()


@pytest.mark.parametrize("K", [0.0, 2e-6, -3e-6])
def test_lensing_kernel_closed_form(hip, K):
    """rf_lensing_potential against analytic line-of-sight integrals (tests/lensing_closed_form.py): constant, linear
    and quadratic potentials, flat and curved, odd and even sample counts; float64 plan to 1e-11, float32 to 2e-6.
    Independent of the oracle's Simpson restatement (generate.py:397-411)."""
    import lensing_closed_form as lcf
    nx, ny, nz, h = 8, 8, 64, 2.5
    for dtype, ct, tol in ((np.float64, np.complex128, 1e-11), (np.float32, np.complex64, 2e-6)):
        plan = hip.DevicePlan(nx, ny, nz, ct)
        for coeffs in ([1.5], [0.2, -0.01], [1.0, 0.03, -2e-4]):
            for i_min in (1, 2, 9):
                DC, DA = lcf.tables(nz, h, K)
                phi = np.polynomial.Polynomial(coeffs)(DC)
                plan.upload_real(np.ascontiguousarray(np.broadcast_to(phi, (nx, ny, nz)), dtype=dtype))
                plan.lensing_potential(cpu_ref.cot_k(DC, DA, K), h, i_min)
                psi = plan.download_aux()
                want = lcf.expected(coeffs, nz, h, i_min)
                assert np.max(np.abs(psi - want[None, None, :])) <= tol * np.max(np.abs(want))
        plan.close()


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("shape", [(64, 32, 128), (1024, 8, 32), (512, 16, 64), (16, 16, 16), (2048, 8, 32),
                                   (16, 16, 512), (1024, 8, 512)])     # nz >= 512: float32 potential rows of nz/2 + 64 cells
def test_fused_potential_store_native(hip, dpower, shape, dtype):
    """rf_realise_potential = the reference's default generate_delta_field(save_potential=True) (generate.py:191-219) with
    the native generator: delta(k)/k**2 written by the generation pass itself.  The field must be the one rf_realise
    gives (to float32 rounding), and the potential the oracle's delta(k)/k**2 of the same noise (float32 generation: 1e-5 of the
    largest magnitude; the unfused route generate -> save_potential agrees with it to the same bound)."""
    k, Pk = dpower
    nx, ny, nz = shape
    plan = make_plan(hip, shape, dtype, k, Pk)     # float64 plans: same float32 generation, values (and the store) widened
    plan.realise(seed=77)
    d0 = plan.download_real()
    std = plan.moments()[1]
    plan.realise_potential(seed=77)
    # same cells, same draws; another kernel instantiation may contract multiply-adds differently (and at nx = 2048 / float64
    # nx = 1024 the plain call transforms x as two half-length transforms, the storing call as one: FFT rounding, 2e-6)
    assert np.max(np.abs(plan.download_real() - d0)) <= 2e-6 * std
    plan.realise_potential(seed=77)
    d1 = plan.download_real()
    plan.realise_potential(seed=77)
    assert np.array_equal(plan.download_real(), d1)               # run-to-run deterministic
    plan.load_potential(1.0)
    pot = plan.download_k()
    noise = cpu_ref.native_noise(77, nx, ny, nz, dtype)
    kref = cpu_ref.generate_kspace(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=np.complex128)
    ref = cpu_ref.potential_kspace(kref, SPACING)
    scale = np.max(np.abs(ref))
    assert pot.shape == ref.shape and pot[0, 0, 0] == 0 and pot.dtype == dtype
    assert np.max(np.abs(pot - ref)) <= 1e-5 * scale
    # the Newtonian potential from it: inverse transform of scale * potential
    plan.load_potential(-2.0)
    plan.execute_c2r()
    phi = plan.download_real()
    want = np.fft.irfftn(-2.0 * ref, s=(nx, ny, nz), axes=(0, 1, 2))
    assert np.max(np.abs(phi - want)) <= 1e-5 * want.std()
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((64, 32, 128), np.complex64), ((1024, 8, 32), np.complex64), ((2048, 8, 32), np.complex64),
                                         ((512, 16, 64), np.complex128), ((1024, 8, 32), np.complex128), ((16, 16, 16), np.complex64),
                                         ((16, 16, 512), np.complex64), ((1024, 8, 512), np.complex64)])     # the padded potential pitch
def test_regenerated_potential_equals_stored_one(hip, dpower, shape, dtype):
    """rf_realise_scaled_potential: calculate_newtonian_potential (generate.py:333-343) with delta(k)/k**2 formed again inside the
    generation pass instead of read from a stored array -- against the stored route (rf_realise_potential, rf_load_potential,
    rf_execute_c2r), which the tests above pin to the oracle.  Native generator on float32 and float64 plans, and the replayed
    reference stream (float32 pairs) on float32 plans."""
    k, Pk = dpower
    nx, ny, nz = shape
    plan = make_plan(hip, shape, dtype, k, Pk)
    scale = -2.5e-3
    for noise in (None, "resident"):
        if noise is not None:
            if dtype == np.complex128:
                assert not plan.can_regenerate_potential("resident")          # float64 plans keep float64 deviates: stored route
                continue
            plan.reference_noise(99, single=True)
        assert plan.can_regenerate_potential(noise)
        plan.realise_potential(seed=77, noise=noise)
        plan.load_potential(scale)
        plan.execute_c2r()
        want = plan.download_real()
        plan.realise(seed=5, noise=noise)                                     # (something else in the field buffer)
        plan.realise_scaled_potential(seed=77, noise=noise, scale=scale)
        got = plan.download_real()
        # (float64 plans draw in float32 arithmetic: two kernel instantiations may round a few deviates differently in the last
        # float32 bit -- measured 1.5e-11 of the rms; the transform itself is float64)
        assert np.max(np.abs(got - want)) <= (2e-6 if dtype == np.complex64 else 1e-9) * want.std()
        assert abs(plan.moments()[1] - want.std()) <= 1e-5 * want.std()
        # the light-cone factor per plane z in the z pass's store: what rf_scale_z makes of the finished field (same roundings
        # on paper; the z pass is another kernel instantiation, so the last float32 bit of its butterflies may differ)
        fz = np.exp(-0.01 * np.arange(nz)) / (1 + 0.002 * np.arange(nz))
        plan.scale_z(fz)
        two_steps = plan.download_real()
        plan.realise_scaled_potential(seed=77, noise=noise, scale=scale, factor_z=fz)
        assert np.max(np.abs(plan.download_real() - two_steps)) <= (1e-6 if dtype == np.complex64 else 1e-13) * two_steps.std()
        assert abs(plan.moments()[1] - two_steps.astype(np.float64).std()) <= 1e-5 * two_steps.std()
    plan.set_exact_generation(True)
    assert not plan.can_regenerate_potential(None)
    with pytest.raises(RuntimeError):
        plan.realise_scaled_potential(seed=77, scale=scale)
    plan.close()


def test_light_cone_factor_survives_a_flag_set_just_before_the_call(hip, dpower):
    """rf_realise_scaled_potential(factor_z) decides where the per-z factor is applied (the plain z pass's store, or a sweep behind
    the gathering z pass of the blocked intermediate) from the plan's FLAG, not from whether the lazily allocated intermediate
    exists yet: with RF_FLAG_TRANSPOSED_INTERMEDIATE set straight before the call -- the plan's first use of it -- the factor used
    to be dropped silently (the result was the z = 0 potential)."""
    k, Pk = dpower
    n = 64
    scale = -2.5e-3
    fz = np.exp(-0.01 * np.arange(n)) / (1 + 0.002 * np.arange(n))
    plan = make_plan(hip, (n, n, n), np.complex64, k, Pk)
    plan.realise_scaled_potential(seed=77, scale=scale, factor_z=fz)
    want = plan.download_real()
    plan.realise_scaled_potential(seed=77, scale=scale)
    plain = plan.download_real()
    assert np.max(np.abs(want - plain * fz.astype(np.float32))) <= 1e-6 * want.std()
    plan.close()
    for first_call in (True, False):
        plan = make_plan(hip, (n, n, n), np.complex64, k, Pk)
        if not first_call:
            plan.realise(seed=1)                                   # (the plan has run without the intermediate before)
        plan.set_transposed_intermediate(True)
        plan.realise_scaled_potential(seed=77, scale=scale, factor_z=fz)
        got = plan.download_real()
        assert np.max(np.abs(got - want)) <= 2e-6 * want.std(), "light-cone factor lost (first call: %s)" % first_call
        plan.set_transposed_intermediate(False)                    # and back: fused into the plain z pass again
        plan.realise_scaled_potential(seed=77, scale=scale, factor_z=fz)
        assert np.max(np.abs(plan.download_real() - want)) <= 2e-6 * want.std()
        plan.close()


def test_generator_regenerates_the_potential_on_demand(hip):
    """Generator: the default call (save_potential=True) without the store, calculate_newtonian_potential from the seed (native)
    or the resident deviates (reference), against Generator(store_potential=True); potential.download() still delivers
    delta(k)/k**2."""
    from randomfield_amd import Generator
    from randomfield_amd.generate import _RegeneratedPotential, _DevicePotential
    nz = 64
    z = np.linspace(0, 0.1, nz)
    kw = dict(growth_function=np.exp(-z), mean_matter_density=1 + z, redshifts=z, transverse_distance=np.arange(nz) * 2.5)
    for rng_kind in ("native", "reference"):
        lazy = Generator(32, 64, nz, 2.5, rng=rng_kind, **kw)
        eager = Generator(32, 64, nz, 2.5, rng=rng_kind, store_potential=True, **kw)
        a = lazy.generate_delta_field(seed=11).copy()
        b = eager.generate_delta_field(seed=11).copy()
        assert isinstance(lazy.potential, _RegeneratedPotential) and isinstance(eager.potential, _DevicePotential)
        assert np.max(np.abs(a - b)) <= 1e-6 * b.std()
        pa, pb = lazy.calculate_newtonian_potential(scale=-1.5).copy(), eager.calculate_newtonian_potential(scale=-1.5).copy()
        assert np.max(np.abs(pa - pb)) <= 2e-6 * pb.std()
        assert np.max(np.abs(lazy.calculate_lensing_potential() - eager.calculate_lensing_potential())) <= 1e-5 * np.abs(pb).max() * nz
        ka, kb = lazy.potential.download(), eager.potential.download()
        assert np.max(np.abs(ka - kb)) <= 2e-6 * np.abs(kb).max()
        lazy.plan_c2r.device.close()
        eager.plan_c2r.device.close()


def test_config5_float64_lognormal_full_size(hip, dpower):
    """BASELINE config 5 at its own size: 1024^3 float64 realisation + apply_lognormal_transform with a growth function
    along z (cosmotools.py:206-221, generate.py:268-273).  Checked through x-planes: the mapped plane equals the oracle's
    map of the downloaded Gaussian plane (1e-13), is positive, and has mean one within sampling noise; the Gaussian field
    itself has zero mean and the rms the float32 run of the same power spectrum has."""
    from randomfield_amd import cosmotools
    n = 1024
    k, Pk = dpower
    try:
        plan = make_plan(hip, (n, n, n), np.complex128, k, Pk)
    except RuntimeError as e:
        pytest.skip("1024^3 float64 does not fit this device: %s" % e)
    plan.realise(seed=5)
    mean, std = plan.moments()
    assert abs(mean) < 1e-9 and abs(std - 2.3137) < 5e-3
    growth = np.exp(-0.5 * np.arange(n) / n)
    before = {x: plan.download_real(x0=x, x1=x + 1).copy() for x in (0, 511, 1023)}
    a_z, b_z = cosmotools.lognormal_tables(growth, std, n)
    plan.lognormal(a_z, b_z, std)
    for x, g in before.items():
        got = plan.download_real(x0=x, x1=x + 1)
        want = cpu_ref.lognormal(g.copy(), growth, sigma=std)
        assert got.dtype == np.float64 and np.all(got > 0)
        assert np.max(np.abs(got - want) / want) <= 1e-12
        assert abs(got.mean() - 1.0) < 0.02
    # the same configuration fused (rf_realise_lognormal): sigma from the y pass (Parseval), the map in the z pass's epilogue
    dens = 1.0 + 0.25 * np.arange(n) / n
    plan.set_z_tables(growth, dens)
    sigma = plan.realise_lognormal(seed=5)
    assert abs(sigma - std) <= 1e-13 * std                      # device sigma (Parseval) == rf_moments' sigma of the Gaussian field
    mean_rho, std_rho = plan.moments()                           # (now the moments of the density field)
    for x, g in before.items():
        got = plan.download_real(x0=x, x1=x + 1)
        want = cpu_ref.scale_z(cpu_ref.lognormal(g.copy(), growth, sigma=sigma), dens)
        assert got.dtype == np.float64 and np.all(got > 0)
        assert np.max(np.abs(got - want) / want) <= 1e-12
    assert abs(mean_rho - dens.mean()) < 0.02
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((64, 64, 128), np.complex64), ((64, 64, 128), np.complex128), ((256, 256, 256), np.complex64),
                                         ((16, 32, 64), np.complex128), ((512, 256, 1024), np.complex64)])
def test_fused_lognormal_realisation(hip, dpower, shape, dtype):
    """rf_realise_lognormal == rf_realise -> rf_moments -> rf_lognormal -> rf_scale_z: sigma from Parseval equals the rms of
    the Gaussian field (float64: 1e-13; float32: the float32 rounding of it), and the density field equals the oracle's map
    of the unfused Gaussian field (float64: 1e-12; float32: 3e-6 = an ulp of expf and of its argument), with native and with host-supplied deviates."""
    k, Pk = dpower
    nx, ny, nz = shape
    f64 = dtype == np.complex128
    plan = make_plan(hip, shape, dtype, k, Pk)
    growth = np.exp(-0.5 * np.arange(nz) / nz)
    dens = 0.5 + np.arange(nz) / nz
    for noise in (None, cpu_ref.reference_noise(11, nx * ny * (nz // 2 + 1))):
        for density in (None, dens):
            plan.realise(seed=21, noise=noise)
            delta = plan.download_real()
            mean, std = plan.moments()
            plan.set_z_tables(growth, density)
            sigma = plan.realise_lognormal(seed=21, noise=noise)
            rho = plan.download_real()
            if f64:
                assert abs(sigma - std) <= 1e-13 * std
            else:
                assert abs(sigma - std) <= 1e-6 * std and sigma == float(np.float32(sigma))    # np.std of float32 data is a float32
            want = cpu_ref.lognormal(delta.copy(), growth, sigma=delta.dtype.type(sigma))
            if density is not None:
                want = cpu_ref.scale_z(want, density)
            assert rho.dtype == delta.dtype and np.all(rho > 0)
            assert np.max(np.abs(rho - want) / want) <= (1e-12 if f64 else 3e-6)     # (float32: expf ulp + |x| * float32 rounding of the field)
            m2, s2 = plan.moments()
            assert abs(m2 - rho.astype(np.float64).mean()) <= 1e-9 and abs(s2 - rho.astype(np.float64).std()) <= 1e-6 * s2
    with pytest.raises(RuntimeError):
        hip.DevicePlan(16, 16, 16).realise_lognormal(seed=1)         # tables first
    plan.close()


def _call_native(plan):
    plan.realise(seed=21)


def _call_resident32(plan):
    plan.reference_noise(99, single=True)
    assert plan.can_regenerate_potential("resident")                 # (the float32 pairs, not the float64 fallback of a short segment)
    plan.realise(noise="resident")


def _call_potential(plan):
    plan.realise_potential(seed=22)


def _call_scaled_potential(plan):
    plan.realise_scaled_potential(seed=23, scale=-2.5e-3, factor_z=np.exp(-0.01 * np.arange(plan.nz)))


def _call_lognormal(plan):
    return plan.realise_lognormal(seed=24)


def _call_batch(plan):
    return tuple(plan.realise_batch([25, 26]))


def _call_refused(plan):
    with pytest.raises(RuntimeError):
        plan.realise(noise="resident")                               # no deviates on this plan (yet)


_CALLS = [_call_native, _call_resident32, _call_potential, _call_scaled_potential, _call_lognormal, _call_batch]


def test_one_call_leaves_nothing_behind_for_the_next(hip, dpower):
    """What one entry point asks of the passes (resident deviates, the scaled potential and its scale, the z table of the z pass,
    the target of the stored potential) belongs to that call alone: for every ordered pair (A, B) of realise (native; resident
    float32 pairs), realise_potential, realise_scaled_potential(factor_z), realise_lognormal, realise_batch and -- as A only -- a
    refused realise(noise='resident'), B straight after A on one plan gives bit for bit the field, the moments and the return
    value that B gives as the first call of a plan."""
    from randomfield_amd import powertools
    k, Pk = dpower
    n = 64
    kgrid = powertools.ksq_axes(n, n, n, SPACING)
    table = cpu_ref.sigma_table(k, Pk, n, n, n, SPACING)
    growth, dens = np.exp(-0.5 * np.arange(n) / n), 0.5 + np.arange(n) / n

    def run(calls):
        plan = hip.DevicePlan(n, n, n, np.complex64)
        plan.set_kgrid(*kgrid)
        plan.set_power(*table)
        plan.set_z_tables(growth, dens)
        for call in calls:
            ret = call(plan)
        out = (ret, plan.moments(), plan.download_real())
        plan.close()
        return out

    fresh = [run([b]) for b in _CALLS]
    for a in _CALLS + [_call_refused]:
        for b, want in zip(_CALLS, fresh):
            ret, moments, field = run([a, b])
            what = "%s after %s" % (b.__name__, a.__name__)
            assert ret == want[0] and moments == want[1], what
            assert np.array_equal(field, want[2]), what


def test_fused_lognormal_ignores_and_preserves_the_blocked_intermediate(hip, dpower):
    """rf_realise_lognormal runs its accumulating y pass in place on W, whatever RF_FLAG_TRANSPOSED_INTERMEDIATE says: on a plan that
    has allocated the blocked intermediate X it gives the flag-off plan's density field and sigma bit for bit, and the plain
    realisation that follows goes through X as the one before did."""
    k, Pk = dpower
    n, seed = 64, 21
    growth, dens = np.exp(-0.5 * np.arange(n) / n), 0.5 + np.arange(n) / n
    plain = make_plan(hip, (n, n, n), np.complex64, k, Pk)
    plain.set_z_tables(growth, dens)
    sigma = plain.realise_lognormal(seed=seed)
    want, want_moments = plain.download_real(), plain.moments()
    plan = make_plan(hip, (n, n, n), np.complex64, k, Pk)
    plan.set_z_tables(growth, dens)
    plan.set_transposed_intermediate(True)
    plan.realise(seed=seed)
    assert plan.nbytes > plain.nbytes                       # (X is there)
    first, first_moments = plan.download_real(), plan.moments()
    assert plan.realise_lognormal(seed=seed) == sigma
    assert np.array_equal(plan.download_real(), want) and plan.moments() == want_moments
    plan.realise(seed=seed)
    assert np.array_equal(plan.download_real(), first) and plan.moments() == first_moments
    plain.close()
    plan.close()


def test_reference_rng_array_and_none_seeds(hip, dpower):
    """random.py:24 hands the seed to np.random.RandomState: array seeds (init_by_array) and None are replayed on the
    GPU like integer seeds -- no host deviates are drawn or uploaded."""
    from randomfield_amd import Generator
    k, Pk = dpower
    n = 32
    gen = Generator(n, n, n, SPACING)
    for seed in ([1, 2, 3], np.arange(700) * 7 + 1, np.array([77])):
        d = gen.generate_delta_field(seed=seed, save_potential=False).copy()
        noise = np.random.RandomState(seed).normal(size=2 * n * n * (n // 2 + 1))
        ref, rms = cpu_ref.generate_delta_field(n, n, n, SPACING, k, Pk, noise=noise)
        assert np.max(np.abs(d - ref)) <= TOL_F32 * rms
    a = gen.generate_delta_field(seed=None, save_potential=False).copy()
    b = gen.generate_delta_field(seed=None, save_potential=False)
    assert np.isfinite(a).all() and not np.array_equal(a, b)
    with pytest.raises(ValueError):
        gen.generate_delta_field(seed=2 ** 32)
    gen.plan_c2r.device.close()


# ---- non-power-of-two grids: the generic mixed-radix kernels (csrc/rf_generic.h) ---------------------------------
# (the generation rows need nz % 4 == 0 -- transform.py:53-56 wants an odd packed last axis; plans take any even nz)
GENERIC_SHAPES = [(40, 60, 80), (10, 14, 24), (12, 18, 8), (26, 34, 44), (24, 8, 16), (2, 2, 4), (6, 1000, 20)]


@pytest.mark.parametrize("shape", GENERIC_SHAPES)
def test_generic_shapes_against_oracle(hip, dpower, shape):
    """Any even shape runs on the GPU (transform.py:172-177 asks for nothing more; (40, 60, 80) is the shape of the
    reference's tests/test_random.py:12-22): same-noise field, rms, k-space, forward transform and the native
    generator's field against the oracle / numpy, float32 and float64 (tests/test_gpu_generic.py does the same on grids where
    every pass has many workgroups)."""
    nx, ny, nz = shape
    k, Pk = dpower
    spacing = 2.5 if max(shape) <= 100 else 0.5                  # keep the grid's k range inside the table
    noise = cpu_ref.reference_noise(11, nx * ny * (nz // 2 + 1))
    for dtype, tol in ((np.complex64, TOL_F32), (np.complex128, TOL_F64)):
        ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, spacing, k, Pk, noise=noise, dtype=dtype, double_fft=True)
        plan = make_plan(hip, shape, dtype, k, Pk, spacing=spacing)
        plan.realise(noise=noise)
        d = plan.download_real()
        assert d.shape == shape and np.max(np.abs(d - ref)) <= tol * rms
        mean, std = plan.moments()
        assert abs(std - rms) <= tol * rms
        ks = plan.download_k()                                   # the generic path materialises k space
        kref = cpu_ref.generate_kspace(nx, ny, nz, spacing, k, Pk, noise=noise, dtype=dtype)
        assert np.max(np.abs(ks - kref)) <= (5e-7 if dtype == np.complex64 else 1e-14) * np.max(np.abs(kref))
        assert cpu_ref.is_hermitian_packed(ks, rtol=0, atol=0)
        # forward transform of the field: back to the same k space (np.fft.rfftn normalisation)
        plan.execute_r2c()
        back = plan.download_k()
        assert np.max(np.abs(back - kref)) <= 20 * tol * np.max(np.abs(kref))
        # native generator: value by value against the oracle's restatement of the same stream (the default fast flavour at
        # 1e-5 * rms, the exact chain at the dtype's tolerance), and deterministic
        nnoise = cpu_ref.native_noise(3, nx, ny, nz, dtype)
        nref, nrms = cpu_ref.generate_delta_field(nx, ny, nz, spacing, k, Pk, noise=nnoise, dtype=dtype, double_fft=True)
        plan.realise(seed=3)
        a = plan.download_real()
        assert np.max(np.abs(a - nref)) <= 1e-5 * nrms and abs(plan.moments()[1] - nrms) <= 1e-5 * nrms
        plan.realise(seed=3)
        assert np.array_equal(a, plan.download_real())
        plan.set_exact_generation(True)
        plan.realise(seed=3)
        assert np.max(np.abs(plan.download_real() - nref)) <= tol * nrms
        plan.set_exact_generation(False)
        rms_b = plan.realise_batch([3, 4, 5])
        assert abs(rms_b[0] - float(np.std(a.astype(np.float64)))) <= 10 * tol * rms and len(set(rms_b)) == 3
        plan.close()


@pytest.mark.parametrize("shape", [(40, 60, 80), (16384, 4, 8), (4, 9000, 8), (4, 6, 16400)])
def test_generic_shape_generator_api(hip, dpower, shape):
    """The drop-in Generator at the reference's (40, 60, 80) -- and on grids with one axis in the four-step form (x, y, and the
    contiguous axis of the packed plan: nz / 2 = 8200 points): default call (save_potential=True, the reference's
    stream replayed on the GPU), Newtonian potential, density and lensing against this repo's numpy backend, which
    is pinned to the reference on the CPU."""
    from randomfield_amd import Generator
    nx, ny, nz = shape
    z = np.linspace(0, 0.1, nz)
    kw = dict(growth_function=np.exp(-z), mean_matter_density=1 + z, redshifts=z,
              transverse_distance=np.arange(nz) * 2.5)
    dev = Generator(nx, ny, nz, 2.5, **kw)
    cpu = Generator(nx, ny, nz, 2.5, backend="numpy", **kw)
    a = dev.generate_delta_field(seed=21).copy()
    b = cpu.generate_delta_field(seed=21).copy()
    rms = float(cpu.delta_field_rms)
    assert a.shape == (nx, ny, nz) and np.max(np.abs(a - b)) <= TOL_F32 * rms
    assert abs(float(dev.delta_field_rms) - rms) <= TOL_F32 * rms
    assert np.max(np.abs(dev.potential.download() - cpu.potential)) <= 1e-6 * np.max(np.abs(cpu.potential))
    pa = dev.calculate_newtonian_potential(scale=-1.5).copy()
    pb = cpu.calculate_newtonian_potential(scale=-1.5).copy()
    assert np.max(np.abs(pa - pb)) <= TOL_F32 * pb.std()
    la, lb = dev.calculate_lensing_potential(), cpu.calculate_lensing_potential()
    assert np.max(np.abs(la - lb)) <= 2e-5 * np.abs(lb).max()
    dev.generate_delta_field(seed=21, save_potential=False)
    cpu.generate_delta_field(seed=21, save_potential=False)
    ra, rb = dev.convert_delta_to_density(), cpu.convert_delta_to_density()
    assert np.max(np.abs(ra - rb) / rb) <= 1e-4


def test_generic_shape_plans(hip):
    """transform.Plan on the hip backend at the reference's test shape (4, 6, 8) and at (40, 60, 80): packed c2r / r2c
    round trip and unpacked c2c, the cases of tests/test_transform.py:150-300."""
    from randomfield_amd.transform import Plan, symmetrize
    from randomfield_amd import cosmotools
    rng = np.random.RandomState(8)
    # nz = 2 (mod 4): the z-table kernels must not let a vector straddle two rows (rows L of a (10, 14, 22) plan)
    dp = hip.DevicePlan(10, 14, 22)
    f = rng.normal(size=(10, 14, 22)).astype(np.float32)
    z = np.linspace(0, 0.1, 22)
    dp.upload_real(f, padded=False)
    dp.lognormal(*cosmotools.lognormal_tables(np.exp(-z), 1.5, 22), 1.5)
    ref = cpu_ref.lognormal(f.copy(), np.exp(-z), sigma=np.float32(1.5))
    assert np.max(np.abs(dp.download_real() - ref) / ref) <= 1e-5
    dp.upload_real(f, padded=False)
    dp.affine_z(np.exp(-z), 1.0)
    dp.scale_z(1 + z)
    ref = (f.astype(np.float64) * np.exp(-z) + 1) * (1 + z)
    assert np.max(np.abs(dp.download_real() - ref)) <= 1e-5 * np.abs(ref).max()
    dp.close()
    # the same three maps on a float64 plan of that shape (vectors of two doubles) and on a float32 generic plan whose nz % 4 == 0
    # selects the 4-wide kernels.  lognormal: relative 1e-12 (float64: test_config5_float64_lognormal_full_size's bound for
    # rf_lognormal) / 1e-5 (float32: the bound above).  affine_z then scale_z against the float64 expression: each call rounds its
    # result once to the plan's dtype, float32 plans round the table entry and the product besides -- under 2.5 eps of the largest
    # magnitude in all; the bound is 4 eps
    for shape, ct, ln_tol in (((10, 14, 22), np.complex128, 1e-12), ((12, 10, 20), np.complex64, 1e-5)):
        nz = shape[2]
        dp = hip.DevicePlan(*shape, ct)
        rt = dp.real_dtype.type
        assert not dp.tiled and (nz % 4 == 0) == (ct == np.complex64)
        f = np.random.RandomState(nz).normal(size=shape).astype(rt)          # (a stream of its own: the plans below keep their inputs)
        z = np.linspace(0, 0.1, nz)
        dp.upload_real(f, padded=False)
        dp.lognormal(*cosmotools.lognormal_tables(np.exp(-z), 1.5, nz), 1.5)
        ref = cpu_ref.lognormal(f.copy(), np.exp(-z), sigma=rt(1.5))
        got = dp.download_real()
        assert got.dtype == rt and got.shape == shape and np.max(np.abs(got - ref) / ref) <= ln_tol
        dp.upload_real(f, padded=False)
        dp.affine_z(np.exp(-z), 1.0)
        ref = f.astype(np.float64) * np.exp(-z) + 1
        got = dp.download_real()
        assert got.dtype == rt and np.max(np.abs(got - ref)) <= 4 * np.finfo(rt).eps * np.abs(ref).max()
        dp.scale_z(1 + z)
        ref = ref * (1 + z)
        assert np.max(np.abs(dp.download_real() - ref)) <= 4 * np.finfo(rt).eps * np.abs(ref).max()
        dp.close()
    for shape in ((4, 6, 8), (40, 60, 80), (10, 14, 22), (12, 18, 6)):
        nx, ny, nz = shape
        for ct, tol in ((np.complex64, 2e-6), (np.complex128, 1e-14)):
            plan = Plan(shape=shape, dtype_in=ct)
            assert plan.backend == "hip"
            rt = plan.data_out.dtype
            plan.data_in.view(rt).reshape(nx, ny, nz + 2)[:] = rng.normal(size=(nx, ny, nz + 2))
            ks = plan.data_in.copy()
            out = plan.execute().copy()
            ref = np.fft.irfftn(ks.astype(np.complex128), s=shape, axes=(0, 1, 2))
            assert np.max(np.abs(out - ref)) <= 10 * tol * ref.std()
            rev = plan.create_reverse_plan()
            back = rev.execute()
            kref = np.fft.rfftn(ref)
            assert np.max(np.abs(back - kref)) <= 20 * tol * np.abs(kref).std()
            for inverse, fn in ((True, np.fft.ifftn), (False, np.fft.fftn)):
                c = Plan(shape=shape, dtype_in=ct, packed=False, inverse=inverse)
                c.data_in[:] = rng.normal(size=shape) + 1j * rng.normal(size=shape)
                src = c.data_in.copy()
                ref = fn(src.astype(np.complex128))
                assert np.max(np.abs(c.execute() - ref)) <= 10 * tol * np.abs(ref).std()


@pytest.mark.parametrize("shape,ct", [((4096, 8, 16), np.complex64), ((8, 8192, 12), np.complex64), ((6, 8, 8192), np.complex64),
                                      ((12, 6000, 8), np.complex64), ((4096, 4, 8), np.complex128), ((4, 6, 4096), np.complex128),
                                      # one axis too long for a line of the LDS: the four-step form (two passes of sub-lines)
                                      ((16384, 4, 8), np.complex64), ((4, 24000, 8), np.complex64), ((4, 6, 40000), np.complex64),
                                      ((6, 4, 32768), np.complex64), ((8192, 4, 8), np.complex128), ((4, 10000, 8), np.complex128),
                                      ((4, 6, 16384), np.complex128), ((4100, 2, 8200), np.complex128)])      # (the last: two long axes at once)
def test_axes_longer_than_2048(hip, dpower, shape, ct):
    """transform.py:172-177 accepts any even shape.  Axes beyond the tiled kernels' 2048 run on the generic mixed-radix kernels with
    the whole line in LDS: up to 8192 complex64 / 4096 complex128 points; longer axes as two passes over factors that fit (the
    four-step form, rf_generic.h).  Packed c2r against numpy's irfftn, the r2c reverse plan, unpacked c2c both ways, and a
    Generator field against the oracle's realisation of the same deviates."""
    from randomfield_amd.transform import Plan
    from randomfield_amd import Generator
    rng = np.random.RandomState(17)
    nx, ny, nz = shape
    tol = 2e-6 if ct == np.complex64 else 1e-14
    plan = Plan(shape=shape, dtype_in=ct)
    assert plan.backend == "hip" and not plan.device.tiled
    rt = plan.data_out.dtype
    plan.data_in.view(rt).reshape(nx, ny, nz + 2)[:] = rng.normal(size=(nx, ny, nz + 2))
    ks = plan.data_in.copy()
    out = plan.execute().copy()
    ref = np.fft.irfftn(ks.astype(np.complex128), s=shape, axes=(0, 1, 2))
    assert np.max(np.abs(out - ref)) <= 20 * tol * ref.std()
    back = plan.create_reverse_plan().execute()
    kref = np.fft.rfftn(ref)
    assert np.max(np.abs(back - kref)) <= 40 * tol * np.abs(kref).std()
    plan.device.close()
    for inverse, fn in ((True, np.fft.ifftn), (False, np.fft.fftn)):
        c = Plan(shape=shape, dtype_in=ct, packed=False, inverse=inverse)
        c.data_in[:] = rng.normal(size=shape) + 1j * rng.normal(size=shape)
        src = c.data_in.copy()
        ref = fn(src.astype(np.complex128))
        assert np.max(np.abs(c.execute() - ref)) <= 20 * tol * np.abs(ref).std()
        c.device.close()
    k, Pk = dpower                                   # (the shipped default power: what Generator() loads)
    spacing = SPACING if max(shape) <= 16384 else 1.0          # (the default power table starts at k = 1e-4: longer boxes need smaller cells)
    gen = Generator(nx, ny, nz, spacing, backend="hip")
    if ct == np.complex64:
        delta = gen.generate_delta_field(seed=4, save_potential=False)
        want, rms = cpu_ref.generate_delta_field(nx, ny, nz, spacing, k, Pk, seed=4, double_fft=True)
        assert delta.shape == shape and np.max(np.abs(delta - want)) <= TOL_F32 * rms
        assert abs(float(gen.delta_field_rms) - rms) <= TOL_F32 * rms
        gen.plan_c2r.device.close()


# ---- the reference's default call and its own random stream on kz-slab ranks (virtual ranks on one device) --------
def _slab_plans(hip, shape, dtype, k, Pk, nranks, exact=False):
    from randomfield_amd import powertools
    nx, ny, nz = shape
    plans = []
    for r in range(nranks):
        p = hip.DevicePlan(nx, ny, nz, dtype, nranks=nranks, rank=r)
        p.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
        p.set_power(*cpu_ref.sigma_table(k, Pk, nx, ny, nz, SPACING))
        p.set_exact_generation(exact)
        plans.append(p)
    return plans


def _slab_run(hip, plans, **forward):
    for p in plans:
        p.slab_forward(**forward)
    hip.DevicePlan.slab_exchange_local(plans)
    for p in plans:
        p.slab_backward()
    return np.concatenate([p.download_real() for p in plans], axis=0)


def _slab_side_array(plans, getter, nzc):
    """Assemble the (nx, ny, nz/2+1) array from the ranks' side arrays (own planes, then the Nyquist plane)."""
    from randomfield_amd import slab
    parts = [getter(p) for p in plans]
    assert (parts[0].shape[2] - 1) * len(plans) == nzc
    return slab.assemble_side_array(parts)


@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("shape,dtype,exact", [((64, 32, 128), np.complex64, False), ((32, 64, 64), np.complex64, True),
                                                ((32, 16, 64), np.complex128, False), ((32, 16, 64), np.complex128, True),
                                                ((2048, 8, 128), np.complex64, False), ((1024, 8, 128), np.complex128, False)])
def test_slab_ranks_default_call_and_newtonian_potential(hip, dpower, shape, dtype, exact, nranks):
    """generate_delta_field(save_potential=True) + calculate_newtonian_potential (generate.py:200-217, 282-350) on kz-slab
    ranks: field, saved potential (every rank keeps its planes of delta(k)/k**2; fused second store stream of the
    generation pass for the native float32 generator, generate -> divide -> transform otherwise) and the transform of the
    scaled potential equal the single-rank results."""
    k, Pk = dpower
    nx, ny, nz = shape
    # (float64 plans generate in float32 arithmetic and widen: different kernel instantiations agree to float32 rounding)
    tol = 2e-6 if dtype == np.complex64 else 2e-7
    one = make_plan(hip, shape, dtype, k, Pk)
    one.set_exact_generation(exact)
    one.realise_potential(seed=9)
    ref = one.download_real()
    std = one.moments()[1]
    one.load_potential(1.0)
    pref = one.download_k()
    one.load_potential(-1.5)
    one.execute_c2r()
    phiref = one.download_real()
    plans = _slab_plans(hip, shape, dtype, k, Pk, nranks, exact)
    field = _slab_run(hip, plans, seed=9, source="potential")
    assert np.max(np.abs(field - ref)) <= tol * std
    def pot(p):
        p.load_potential(1.0)
        return p.download_k()
    assert plans[1].k_shape == (nx, ny, nz // 2 // nranks + 1)
    got = _slab_side_array(plans, pot, nz // 2)
    assert np.max(np.abs(got - pref)) <= tol * np.max(np.abs(pref))
    for p in plans:
        p.load_potential(-1.5)
    phi = _slab_run(hip, plans, source="kspace")
    assert np.max(np.abs(phi - phiref)) <= tol * phiref.std()
    # lensing scan along z: rows are local to the x slabs
    cot = 1.0 / (1.0 + np.arange(nz))
    one.lensing_potential(cot, SPACING, 2)
    lref = one.download_aux()
    for p in plans:
        p.lensing_potential(cot, SPACING, 2)
    lens = np.concatenate([p.download_aux() for p in plans], axis=0)
    assert np.max(np.abs(lens - lref)) <= 10 * tol * np.abs(lref).max()
    for p in plans + [one]:
        p.close()


@pytest.mark.parametrize("nranks", [2, 4])
def test_slab_ranks_reference_stream(hip, dpower, nranks):
    """rng='reference' on kz-slab ranks: every rank replays RandomState(seed).normal on the GPU and keeps the deviates of
    its own planes; host-supplied deviates are cut the same way.  Field = the single-rank field = the reference's."""
    k, Pk = dpower
    shape = (32, 32, 64)
    nx, ny, nz = shape
    seed = 321
    noise = cpu_ref.reference_noise(seed, nx * ny * (nz // 2 + 1))
    ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, double_fft=True)
    plans = _slab_plans(hip, shape, np.complex64, k, Pk, nranks)
    for p in plans:
        p.reference_noise(seed)
    got = _slab_side_array(plans, lambda p: p.download_noise().reshape(p.k_shape + (2,)), nz // 2)
    assert np.max(np.abs(got.reshape(-1) - noise) / np.maximum(np.abs(noise), 1e-300)) <= 1e-14   # numpy's stream, value for value
    field = _slab_run(hip, plans, noise="resident")
    assert np.max(np.abs(field - ref)) <= TOL_F32 * rms
    field = _slab_run(hip, plans, noise=noise)                          # host deviates, exact reference chain
    assert np.max(np.abs(field - ref)) <= TOL_F32 * rms
    field = _slab_run(hip, plans, noise="resident", source="potential")  # the default call with the reference's stream
    assert np.max(np.abs(field - ref)) <= TOL_F32 * rms
    def pot(p):
        p.load_potential(1.0)
        return p.download_k()
    kref = cpu_ref.generate_kspace(nx, ny, nz, SPACING, k, Pk, noise=noise)
    from randomfield_amd import powertools
    kx2, ky2, kz2 = powertools.ksq_axes(nx, ny, nz, SPACING)
    k2 = (kx2[:, None, None] + ky2[None, :, None] + kz2[None, None, :]).astype(np.float32)
    k2[0, 0, 0] = np.inf
    assert np.max(np.abs(_slab_side_array(plans, pot, nz // 2) - kref / k2)) <= 2e-6 * np.max(np.abs(kref / k2))
    for p in plans:
        p.close()


@pytest.mark.parametrize("shape,dtype,nranks", [((32, 16, 64), np.complex64, 2), ((64, 32, 128), np.complex64, 4), ((32, 16, 64), np.complex128, 4),
                                                 ((1024, 8, 256), np.complex64, 8), ((16, 2048, 64), np.complex64, 2)])
def test_forward_r2c_on_slab_ranks(hip, shape, dtype, nranks):
    """rf_execute_r2c on multi-rank plans (transform.py:278-301's reverse plan): every rank uploads its x slab, runs the z pass
    on its rows, the all-to-all goes the other way (x slabs -> kz slabs; device copies between virtual ranks), the y and x passes
    run on the kz slab and every rank ends up with its planes (+ the Nyquist plane on rank 0) of np.fft.rfftn.  Then the way back
    through the ordinary inverse pipeline: c2r(r2c(x)) = x."""
    nx, ny, nz = shape
    rt, tol = (np.float32, 3e-6) if dtype == np.complex64 else (np.float64, 1e-13)
    rng = np.random.RandomState(nx + nz)
    f = rng.normal(size=shape).astype(rt)
    ref = np.fft.rfftn(f.astype(np.float64), axes=(0, 1, 2))
    plans = [hip.DevicePlan(nx, ny, nz, dtype, nranks=nranks, rank=r) for r in range(nranks)]
    nxl = nx // nranks
    for r, p in enumerate(plans):
        p.upload_real(np.ascontiguousarray(f[r * nxl:(r + 1) * nxl]))
        p.slab_r2c_rows()
    hip.DevicePlan.slab_exchange_local_reverse(plans)
    for p in plans:
        p.slab_r2c_cols()
    got = _slab_side_array(plans, lambda p: p.download_k(), nz // 2)
    assert got.shape == ref.shape and np.max(np.abs(got - ref)) <= 10 * tol * np.abs(ref).std() * np.sqrt(np.log2(f.size))
    for p in plans[1:]:
        assert np.all(p.download_k()[:, :, -1] == 0)              # (the Nyquist slot of the ranks that do not own it)
    back = _slab_run(hip, plans, source="kspace")
    assert np.max(np.abs(back - f)) <= 20 * tol * f.std()
    for p in plans:
        p.close()


def test_distributed_generator_single_rank(hip, monkeypatch):
    """Generator(distributed=True) with WORLD_SIZE = 1: the per-rank plumbing (SlabHostPlan window, agreed seeds, local
    potential / lensing downloads) gives the ordinary Generator's results.  With more ranks the same calls run the slab
    pipeline that the virtual-rank tests above check step by step."""
    from randomfield_amd import Generator
    for key, val in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")):
        monkeypatch.setenv(key, val)
    nz = 64
    z = np.linspace(0, 0.1, nz)
    kw = dict(growth_function=np.exp(-z), mean_matter_density=1 + z, redshifts=z, transverse_distance=np.arange(nz) * 2.5)
    with pytest.raises(ValueError):
        Generator(32, 32, nz, 2.5, distributed=True, exchange_chunks=0, **kw)      # (opt-in sub-slab exchange: a count >= 1)
    for rng_kind in ("reference", "native"):
        one = Generator(32, 32, nz, 2.5, rng=rng_kind, **kw)
        dist = Generator(32, 32, nz, 2.5, rng=rng_kind, distributed=True, exchange_chunks=(4 if rng_kind == "native" else None), **kw)
        assert dist.plan_c2r.data_out.shape == (32, 32, nz)
        a = one.generate_delta_field(seed=5).copy()
        b = dist.generate_delta_field(seed=5).copy()
        assert np.array_equal(a, b) and one.delta_field_rms == dist.delta_field_rms
        # generate.py:79-80: the forward plan over the same memory.  On a slab rank it takes the rank's window of the field
        # (aliasing the c2r plan's output, as the reference's pair of plans does) and returns the rank's kz planes + Nyquist
        r2c = dist.plan_r2c
        assert r2c is not None and not r2c.inverse and r2c.data_in_padded is dist.plan_c2r.data_out_padded
        assert r2c.data_out.shape == (32, 32, nz // 2 + 1) and r2c.data_out.dtype == np.complex64
        ks = r2c.execute()
        assert ks is r2c.data_out and np.max(np.abs(ks - np.fft.rfftn(b.astype(np.float64)))) <= 2e-5 * np.abs(ks).max()
        assert np.max(np.abs(ks - one.plan_r2c.execute())) <= 1e-6 * np.abs(ks).max()
        with pytest.raises(RuntimeError):
            dist.plan_c2r.execute()
        assert np.array_equal(one.potential.download(), dist.potential.download())
        pa, pb = one.calculate_newtonian_potential(scale=-1.5).copy(), dist.calculate_newtonian_potential(scale=-1.5).copy()
        assert np.array_equal(pa, pb)
        assert np.array_equal(one.calculate_lensing_potential(), dist.calculate_lensing_potential())
        one.generate_delta_field(seed=5, save_potential=False)
        dist.generate_delta_field(seed=5, save_potential=False)
        assert np.array_equal(one.convert_delta_to_density(), dist.convert_delta_to_density())
        assert dist.generate_delta_field(seed=None, save_potential=False).shape == (32, 32, nz)   # agreed seed path


@pytest.mark.parametrize("nranks,single", [(2, False), (4, False), (4, True), (8, True)])
def test_shared_reference_stream_small(hip, dpower, nranks, single):
    """rf_mt_share_*: ONE replay of RandomState(seed).normal shared by the ranks of a kz-slab job (each rank jumps to its own range
    of segments, replays it, one all-to-all of deviates) against numpy's stream itself and against the oracle's field.  Short
    segments (16 blocks) so that a 32 x 32 x 128 stream has 35 of them: ranks whose first segment has one, two and zero non-zero
    radix-16 digits, shares that end inside rows, and a last rank whose share ends with the stream's unused tail."""
    k, Pk = dpower
    shape = (32, 32, 128)
    nx, ny, nz = shape
    plans = _slab_plans(hip, shape, np.complex64, k, Pk, nranks)
    for p in plans:
        p.set_mt_segment_blocks(16)
    nseg, first, count = plans[-1].share_segments()
    assert nseg == 35 and first + count == nseg and plans[0].share_segments()[1] == 0
    for seed in (321, 7):                                               # (the second seed reuses every buffer)
        noise = cpu_ref.reference_noise(seed, nx * ny * (nz // 2 + 1))
        ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, double_fft=True)
        acc = hip.DevicePlan.reference_noise_shared_local(plans, seed, single=single)
        assert len(set(acc)) == 1 and acc[0] >= nx * ny * (nz // 2 + 1)
        parts = [p.download_noise().reshape(p.k_shape + (2,)) for p in plans]
        got = _slab_side_array(plans, lambda p: parts[plans.index(p)], nz // 2)
        # float64 transport: numpy's values to the last bits.  float32 form: every deviate in ITS cell, to 3e-7 of its value or
        # 2e-6 absolute -- the replay's fast path (rf_k_mt.hip) works on float32 x1, x2 between r2 = 2^-9 and 1 - 2^-8: the
        # rounding of r2 = x1^2 + x2^2 (1e-7 absolute, zero mean) is 1e-7 / (1 - r2) of ln r2 there, i.e. up to 1.5e-6 on the
        # SMALL deviates |g| < 0.13 that come from r2 > 0.99; deviates of order one and the tails keep float32 accuracy
        dev = np.abs(got.reshape(-1) - noise)
        if single:
            assert np.max(dev - 3e-7 * np.abs(noise)) <= 2e-6 and np.sqrt(np.mean(dev ** 2)) <= 2e-7
            assert np.max((dev / np.maximum(np.abs(noise), 1e-30))[np.abs(noise) > 0.5]) <= 1e-6
        else:
            assert np.max(dev / np.maximum(np.abs(noise), 1e-300)) <= 1e-14
        for q in parts[1:]:                                             # every rank carries the Nyquist plane
            assert np.array_equal(q[:, :, -1], parts[0][:, :, -1])
        field = _slab_run(hip, plans, noise="resident")
        assert np.max(np.abs(field - ref)) <= TOL_F32 * rms
    for p in plans:
        p.close()


@pytest.mark.parametrize("shape,dtype,nranks", [((256, 256, 256), np.complex64, 8), ((128, 64, 256), np.complex128, 4)])
def test_shared_reference_stream_equals_replicated_replay(hip, dpower, shape, dtype, nranks):
    """Default segment length (68 / 9 segments): the shared replay in float64 mode leaves bit for bit the deviates that the
    replicated replay (every rank replays everything: rf_noise_mt19937_ex on a multi-rank plan) leaves, float32 mode the same
    values rounded as the single-rank float32 replay rounds them; fields agree with the single-rank field of the same seed."""
    k, Pk = dpower
    nx, ny, nz = shape
    seed = 20260101
    one = make_plan(hip, shape, dtype, k, Pk)
    one.reference_noise(seed)
    one.realise(noise="resident")
    ref, rms = one.download_real(), one.moments()[1]
    one.close()
    plans = _slab_plans(hip, shape, dtype, k, Pk, nranks)
    for p in plans:
        p.reference_noise(seed)                                         # replicated: float64 deviates of the own planes
    want = [p.download_noise() for p in plans]
    hip.DevicePlan.reference_noise_shared_local(plans, seed, single=False)
    for p, w in zip(plans, want):
        assert np.array_equal(p.download_noise(), w)
    field = _slab_run(hip, plans, noise="resident")
    assert np.max(np.abs(field - ref)) <= (2e-6 if dtype == np.complex64 else 1e-12) * rms
    if dtype == np.complex64:
        hip.DevicePlan.reference_noise_shared_local(plans, seed, single=True)
        for p, w in zip(plans, want):
            g = p.download_noise()
            assert np.array_equal(g, g.astype(np.float32)) and np.max(np.abs(g - w) - 3e-7 * np.abs(w)) <= 2e-6      # (see test_shared_reference_stream_small)
        field = _slab_run(hip, plans, noise="resident")
        assert np.max(np.abs(field - ref)) <= 3e-6 * rms
    for p in plans:
        p.close()


def test_shared_reference_stream_headline_size_against_reference_summary(hip, dpower):
    """1024^3 over 8 virtual kz-slab ranks, seed 123, the stream replayed ONCE by the eight ranks together (4093 segments, 511-512
    per rank; float32 transport): 4096 field values, the spot values and the rms of the REFERENCE's own run
    (tests/golden/summary_1024_c64.npz, oracle/make_golden_large.py)."""
    g = golden("summary_1024_c64.npz")
    n, P = 1024, 8
    k, Pk = dpower
    plans = _slab_plans(hip, (n, n, n), np.complex64, k, Pk, P)
    nseg = plans[0].share_segments()[0]
    assert nseg >= 4000 and sum(p.share_segments()[2] for p in plans) == nseg
    acc = hip.DevicePlan.reference_noise_shared_local(plans, 123, single=True)
    assert acc[0] >= n * n * (n // 2 + 1)
    for p in plans:
        p.slab_forward(noise="resident")
    hip.DevicePlan.slab_exchange_local(plans)
    tot = np.zeros(2)
    for p in plans:
        p.slab_backward()
        tot += np.array(p.slab_stats())
    rms = float(g["rms"])
    cells = float(n) ** 3
    assert abs(np.sqrt(tot[1] / cells - (tot[0] / cells) ** 2) - rms) <= TOL_F32 * rms
    nxl, s = n // P, n // 16
    row = lambda ix: plans[ix // nxl].download_real(x0=ix % nxl, x1=ix % nxl + 1)[0]
    sub = np.stack([row(ix)[::s, ::s] for ix in range(0, n, s)])
    assert np.max(np.abs(sub - g["sub"])) <= TOL_F32 * rms
    assert np.max(np.abs(row(0)[0, :4] - g["first"])) <= TOL_F32 * rms and np.max(np.abs(row(n - 1)[-1, -4:] - g["last"])) <= TOL_F32 * rms
    for p in plans:
        p.close()


def test_reference_stream_float32_copies(hip, dpower):
    """rf_noise_mt19937_ex(single = 1): the replayed numpy stream kept as float32 pairs (what Generator(complex64,
    rng='reference') uses).  Accept / reject is still float64, so every deviate lands in the same cell; the field, the
    fused potential store and the kz-slab ranks agree with the float64 deviates to 3e-6 * rms (float32 rounding of g,
    log1p near r2 = 1), inside the parity tolerance against the oracle."""
    k, Pk = dpower
    shape = (64, 32, 128)
    nx, ny, nz = shape
    seed = 77
    noise = cpu_ref.reference_noise(seed, nx * ny * (nz // 2 + 1))
    ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, double_fft=True)
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    plan.reference_noise(seed, single=False)
    plan.realise(noise="resident")
    d64 = plan.download_real()
    plan.reference_noise(seed, single=True)
    with pytest.raises(RuntimeError):
        plan.download_noise(0, 4)                                        # only float32 copies are resident now
    with pytest.raises(RuntimeError):
        plan.generate(noise="resident")                                  # the unfused generator reads float64 deviates
    plan.realise(noise="resident")
    d32 = plan.download_real()
    assert np.max(np.abs(d32 - d64)) <= 3e-6 * rms and np.max(np.abs(d32 - ref)) <= TOL_F32 * rms
    assert abs(plan.moments()[1] - rms) <= TOL_F32 * rms
    plan.realise_potential(noise="resident")                             # fused: second store stream of the generation pass
    assert np.max(np.abs(plan.download_real() - ref)) <= TOL_F32 * rms
    plan.load_potential(1.0)
    pot = plan.download_k()
    kref = cpu_ref.generate_kspace(nx, ny, nz, SPACING, k, Pk, noise=noise)
    from randomfield_amd import powertools
    kx2, ky2, kz2 = powertools.ksq_axes(nx, ny, nz, SPACING)
    k2 = (kx2[:, None, None] + ky2[None, :, None] + kz2[None, None, :]).astype(np.float32)
    k2[0, 0, 0] = np.inf
    assert np.max(np.abs(pot - kref / k2)) <= 2e-6 * np.max(np.abs(kref / k2))
    # the exact-generation flag turns the request into float64 deviates (that chain reads nothing else)
    plan.set_exact_generation(True)
    plan.reference_noise(seed, single=True)
    assert np.allclose(plan.download_noise(0, 8), noise[:8], rtol=1e-14, atol=0)
    plan.close()
    plans = _slab_plans(hip, shape, np.complex64, k, Pk, 4)
    for p in plans:
        p.reference_noise(seed, single=True)
    field = _slab_run(hip, plans, noise="resident", source="potential")
    assert np.max(np.abs(field - ref)) <= TOL_F32 * rms
    def slab_pot(p):
        p.load_potential(1.0)
        return p.download_k()
    assert np.max(np.abs(_slab_side_array(plans, slab_pot, nz // 2) - kref / k2)) <= 2e-6 * np.max(np.abs(kref / k2))
    for p in plans:
        p.close()


@pytest.mark.parametrize("shape,dtype", [((256, 256, 256), np.complex64), ((512, 512, 512), np.complex64), ((1024, 1024, 64), np.complex64),
                                         ((64, 2048, 128), np.complex64), ((2048, 64, 256), np.complex64), ((128, 128, 256), np.complex128),
                                         ((1024, 16, 2048), np.complex128), ((512, 256, 1024), np.complex64)])
def test_slabs_and_blocked_intermediate_only_move_data(hip, dpower, shape, dtype):
    """The y / z passes slab by slab (RF_FLAG_YZ_SLAB_PLANES) and the blocked intermediate of the x pass (RF_FLAG_TRANSPOSED_INTERMEDIATE:
    contiguous x-pass chunks, y pass in place on them, gathering z pass) change where data sits between the passes, not the
    field (slabs: not one bit of it): native realisation, uploaded k space and the graph-replayed batch against the whole-grid in-place passes."""
    k, Pk = dpower
    nx, ny, nz = shape
    plan = make_plan(hip, shape, dtype, k, Pk)
    rng = np.random.RandomState(5)
    ks = (rng.normal(size=(nx, ny, nz // 2 + 1)) + 1j * rng.normal(size=(nx, ny, nz // 2 + 1))).astype(dtype)
    cpu_ref.symmetrize_packed(ks)
    seeds = np.array([11, 12, 13], np.uint64)
    res = {}
    for xp, planes in ((0, 0), (0, -1), (0, max(1, nx // 4)), (1, 0), (1, max(1, nx // 4)), (1, -1), (0, max(1, nx // 16))):
        plan.set_transposed_intermediate(bool(xp))
        plan.set_yz_slab_planes(planes)
        plan.realise(seed=99)
        a = plan.download_real()
        ma = plan.moments()
        plan.upload_k(ks)
        plan.execute_c2r()
        b = plan.download_real()
        rms = plan.realise_batch(seeds)
        c = plan.download_real()
        res[(xp, planes)] = (a, b, c, ma, rms)
    a0, b0, c0, m0, r0 = res[(0, 0)]
    assert np.max(np.abs(b0 - np.fft.irfftn(ks.astype(np.complex128), s=shape, axes=(0, 1, 2)))) <= (2e-5 if dtype == np.complex64 else 1e-12) * b0.std()
    for key, (a, b, c, ma, rms) in res.items():
        if key[0] == 0:          # slabs: the same kernels on sub-ranges
            assert np.array_equal(a, a0) and np.array_equal(b, b0) and np.array_equal(c, c0), key
            assert abs(ma[1] - m0[1]) <= 1e-9 * m0[1] and np.max(np.abs(rms - r0)) <= 1e-9 * r0.max(), key
        else:                    # blocked intermediate: the same transform in other kernel instantiations -- float32 rounding apart (the
            # in-place y pass of length 1024 runs as two 512-point transforms per tile, the one on the intermediate as one 1024-point
            # transform; the gathering z pass deals its rows to other threads, which reorders the float32 partial moments)
            for u, v in ((a, a0), (b, b0), (c, c0)):
                assert np.max(np.abs(u - v)) <= (4e-6 if dtype == np.complex64 else 1e-14) * v.std(), key
            assert abs(ma[1] - m0[1]) <= (1e-6 if dtype == np.complex64 else 1e-9) * m0[1], key
            assert np.max(np.abs(rms - r0)) <= (1e-6 if dtype == np.complex64 else 1e-9) * r0.max(), key
    plan.close()


def test_bench_multi_gpu_code_path_with_one_rank(hip):
    """`bench.py --force-multi --full` runs main_multi -- DistributedPlan, the deadline-guarded first exchange, the pipelined slab
    batch, the RCCL all-reduces (a one-rank communicator) -- as a child process on one GPU and prints a well-formed line."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--force-multi", "--steps", "3", "--warmup", "1",
                        "--edge", "256", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["unit"] == "Mcells/s" and line["value"] > 0
    assert line["config"]["grid"] == [256, 256, 256] and 2.0 < line["config"]["rms_last"] < 2.6
    assert line["roofline"]["frac"] > 0 and line["pipeline"]["kernel_ms_rank0_unpipelined_step"]["x"] > 0
    # what RCCL itself says the communicator spans, and the N = 1 equivalent timed in the same job
    assert line["config"]["rccl_ranks"] == 1 and line["config"]["launcher"].startswith("external")
    assert line["single_gpu_equivalent"]["grid"] == [256, 256, 256] and line["single_gpu_equivalent"]["ms_per_step"] > 0
    # both kz-slab modes were calibrated (the direct one reproduced the rccl mode's rms, or it would be listed as rejected) and one runs
    cal = line["config"]["mode_calibration_ms_per_step"]
    assert cal["rccl"] > 0 and cal["direct"] > 0 and line["config"]["modes_rejected"] == {}
    assert line["config"]["multi_gpu_mode"] in ("rccl", "direct") and line["config"]["exchange_sub_slabs"] in (1, 4)
    # ... and the last timed realisation went through the other exchange once more after the timed region: same rms
    cross = line["config"]["exchange_cross_check"]
    assert cross["agree"] is True and cross["other_mode"] != line["config"]["multi_gpu_mode"]
    assert abs(cross["rms_timed_mode"] - line["config"]["rms_last"]) < 1e-5


def test_bench_plain_run_dumps_its_last_timed_field(hip, tmp_path):
    """A plain `bench.py` run (no --full) prints the headline line alone, and --dump-outputs writes what its last timed step computed:
    the sampled cells, the plane x = 0 and the moments of that seed's field realised once more here.  Two runs with the same
    arguments write the same field values."""
    import json
    import subprocess
    import sys
    from randomfield_amd import powertools
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    steps, edge = 3, 256
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--edge", str(edge), "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = lines[0]
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "Mcells/s" and line["config"]["grid"] == [edge] * 3
    assert not {"roofline", "pipeline", "other_configs", "cpu_baseline"} & set(line), "a plain run measures the headline alone"
    names = ["delta_moments.npy", "delta_sample.npy", "delta_sample_index.npy", "delta_x0.npy"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == names
    out = {n[:-4]: np.load(str(tmp_path / "a" / n)) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in out.values()) and sum(v.nbytes for v in out.values()) <= 64 << 20
    for n in ("delta_sample.npy", "delta_sample_index.npy", "delta_x0.npy"):
        assert np.array_equal(np.load(str(tmp_path / "b" / n)), out[n[:-4]]), n
    plan = hip.DevicePlan(edge, edge, edge, np.complex64)
    plan.set_kgrid(*powertools.ksq_axes(edge, edge, edge, 2.5))
    plan.set_power(*powertools.sigma_table(powertools.load_default_power(), (edge, edge, edge), 2.5))
    plan.realise(seed=123 + steps - 1)                                    # the seed of the last timed step
    field = plan.download_real()
    mean, rms = plan.moments()
    plan.close()
    idx = out["delta_sample_index"].astype(np.int64)
    assert len(idx) > 1000 and np.all(np.diff(idx) > 0) and idx[-1] < edge ** 3
    assert np.max(np.abs(out["delta_sample"] - field.reshape(-1)[idx])) <= 1e-6 * rms
    assert np.max(np.abs(out["delta_x0"] - field[0])) <= 1e-6 * rms
    assert abs(out["delta_moments"][1] - rms) <= 1e-6 * rms and abs(out["delta_moments"][0] - mean) <= 1e-6 * rms
    assert abs(line["config"]["rms_last"] - rms) <= 1e-5


def test_bench_multi_gpu_code_path_plain_run_dumps_its_last_timed_field(hip, tmp_path):
    """`bench.py --force-multi` without --full: the slab pipeline's line without the comparators, and --dump-outputs writes the field of
    the last timed realisation (the single-GPU field of that seed)."""
    import json
    import subprocess
    import sys
    from randomfield_amd import powertools
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    steps, edge = 3, 256
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--force-multi", "--steps", str(steps), "--warmup", "1",
                        "--edge", str(edge), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["config"]["multi_gpu_mode"] in ("rccl", "direct")
    assert "single_gpu_equivalent" not in line and "exchange_cross_check" not in line["config"]
    assert "kernel_ms_rank0_unpipelined_step" not in line["pipeline"]
    plan = hip.DevicePlan(edge, edge, edge, np.complex64)
    plan.set_kgrid(*powertools.ksq_axes(edge, edge, edge, 2.5))
    plan.set_power(*powertools.sigma_table(powertools.load_default_power(), (edge, edge, edge), 2.5))
    plan.realise(seed=123 + steps - 1)
    field = plan.download_real()
    mean, rms = plan.moments()
    plan.close()
    idx = np.load(str(tmp_path / "delta_sample_index.npy")).astype(np.int64)
    assert len(idx) > 1000
    assert np.max(np.abs(np.load(str(tmp_path / "delta_sample.npy")) - field.reshape(-1)[idx])) <= 1e-6 * rms
    assert np.max(np.abs(np.load(str(tmp_path / "delta_x0.npy")) - field[0])) <= 1e-6 * rms
    assert abs(np.load(str(tmp_path / "delta_moments.npy"))[1] - rms) <= 1e-6 * rms


def test_two_distributed_plans_in_a_row(hip, dpower, monkeypatch, tmp_path):
    """Two DistributedPlans built one after the other in one process (world 1 here; the rendezvous names differ per plan) give
    the same field as a plain plan."""
    from randomfield_amd import powertools, slab
    monkeypatch.setenv("TMPDIR", str(tmp_path))
    k, Pk = dpower
    n = 64
    ref = make_plan(hip, (n, n, n), np.complex64, k, Pk)
    ref.realise(seed=5)
    want = ref.download_real()
    ref.close()
    paths = []
    for i in range(2):
        d = slab.DistributedPlan(n, n, n, np.complex64, device=0, rank=0, world=1)
        paths.append(d._path)
        d.plan.set_kgrid(*powertools.ksq_axes(n, n, n, SPACING))
        d.plan.set_power(*cpu_ref.sigma_table(k, Pk, n, n, n, SPACING))
        d.plan.realise(seed=5)
        assert np.array_equal(d.plan.download_real(), want)
        d.barrier()
        d.plan.close()
    assert paths[0] != paths[1]


@pytest.mark.parametrize("shape,dtype", [((2048, 2048, 1024), np.complex64), ((1024, 2048, 2048), np.complex128)])
def test_unpacked_c2c_shapes_that_need_64bit_lane_offsets(hip, shape, dtype):
    """The largest unpacked c2c arrays put the rows of the x pass more than 4 GiB apart (34 GB complex64, 69 GB complex128):
    64-bit lane offsets, instantiated for axes >= 1024.  A handful of spikes in, plane waves out (closed form, sampled),
    and the inverse brings the spikes back.  (With axes <= 2048 no shorter axis reaches such strides; rf_plan_create_c2c
    checks it all the same.)"""
    nx, ny, nz = shape
    plan = hip.DevicePlan(nx, ny, nz, dtype, unpacked=True)
    a = np.zeros(shape, dtype)                                   # (lazily mapped: only touched pages cost anything)
    spikes = [((0, 0, 0), 1.0), ((3, 5, 7), 2 - 1j), ((nx - 1, ny // 2, 11), 0.5j), ((nx // 2 + 1, 1, nz - 1), -1.5)]
    for pos, v in spikes:
        a[pos] = v
    plan.upload_c(a)
    plan.execute_c2c(inverse=False)
    plan.download_c(out=a)
    rng = np.random.RandomState(1)
    kk = np.stack([rng.randint(0, n, 4000) for n in shape], axis=1)
    kk[:8] = [[0, 0, 0], [nx - 1, ny - 1, nz - 1], [nx // 2, 0, 0], [0, ny // 2, 0], [0, 0, nz // 2], [nx - 1, 0, 0], [1, 1, 1], [nx // 2, ny // 2, nz // 2]]
    want = np.zeros(len(kk), np.complex128)
    for (x, y, z), v in spikes:
        # (phases reduced modulo one turn in integer arithmetic: k x runs to millions of turns)
        want += v * np.exp(-2j * np.pi * ((kk[:, 0] * x % nx) / nx + (kk[:, 1] * y % ny) / ny + (kk[:, 2] * z % nz) / nz))
    got = a[kk[:, 0], kk[:, 1], kk[:, 2]]
    assert np.max(np.abs(got - want)) <= (2e-5 if dtype == np.complex64 else 1e-12)
    plan.execute_c2c(inverse=True)
    plan.download_c(out=a)
    for pos, v in spikes:
        assert abs(a[pos] - v) <= (2e-6 if dtype == np.complex64 else 1e-13)
        a[pos] = 0
    assert np.max(np.abs(a[kk[:, 0], kk[:, 1], kk[:, 2]])) <= (2e-6 if dtype == np.complex64 else 1e-13)
    plan.close()
    del a


def test_generator_notices_tables_changed_behind_its_back(hip):
    """The 'tables unchanged, skip the upload' shortcut of Generator lives with the device plan: after someone changes the
    tables through the documented ``plan_c2r.device`` handle, the next generate_delta_field uploads its own again."""
    from randomfield_amd import Generator
    gen = Generator(64, 64, 64, SPACING, backend="hip", rng="native")
    a = gen.generate_delta_field(seed=3, save_potential=False).copy()
    dev = gen.plan_c2r.device
    assert dev.set_power(*[np.asarray(t) for t in _other_tables()]) is True       # someone else's tables on the same device plan
    b = gen.generate_delta_field(seed=3, save_potential=False).copy()
    assert np.array_equal(a, b)
    assert dev.set_power(*_other_tables(), if_changed=True) is True               # (and the key follows every upload)
    assert dev.set_power(*_other_tables(), if_changed=True) is False
    dev.close()


def test_regenerated_potential_refuses_a_changed_device_state(hip):
    """A potential that is formed again on demand is a function of the seed, the power tables and (rng='reference') the resident
    deviates.  The reference's stored array cannot change behind the caller's back; ours says so instead of returning the
    potential of some other field when somebody has replaced any of those through ``plan_c2r.device``."""
    from randomfield_amd import Generator
    from randomfield_amd.generate import _RegeneratedPotential
    for rng in ("native", "reference"):
        gen = Generator(64, 64, 64, SPACING, backend="hip", rng=rng)
        dev = gen.plan_c2r.device
        gen.generate_delta_field(seed=3)
        assert isinstance(gen.potential, _RegeneratedPotential)
        want = gen.calculate_newtonian_potential(light_cone=False, scale=-1.5).copy()
        assert np.array_equal(gen.calculate_newtonian_potential(light_cone=False, scale=-1.5), want)      # repeatable while nothing changes
        dev.set_power(*[np.asarray(t) for t in _other_tables()])                     # other tables on the same device plan
        with pytest.raises(RuntimeError, match="power"):
            gen.calculate_newtonian_potential(light_cone=False, scale=-1.5)
        with pytest.raises(RuntimeError, match="power"):
            gen.potential.download()
        gen.generate_delta_field(seed=3)                                             # a new field: its potential is current again
        assert np.max(np.abs(gen.calculate_newtonian_potential(light_cone=False, scale=-1.5) - want)) <= 1e-6 * want.std()
        if rng == "reference":
            dev.reference_noise(4, single=True)                                      # somebody replays another seed's stream
            with pytest.raises(RuntimeError, match="deviates"):
                gen.calculate_newtonian_potential(light_cone=False, scale=-1.5)
        else:
            dev.reference_noise(4, single=True)                                      # (irrelevant to the native generator)
            gen.calculate_newtonian_potential(light_cone=False, scale=-1.5)
        dev.close()


def _other_tables():
    x = np.linspace(-3.0, 1.5, 64)
    return x, 100.0 * np.exp(-0.5 * (x + 1.0) ** 2)


def test_generator_density_field_fused(hip, dpower):
    """Generator.generate_density_field == generate_delta_field(save_potential=False) + convert_delta_to_density(), through the
    fused device call on a tiled single-GPU plan (and through the two reference calls on a generic shape)."""
    from randomfield_amd import Generator
    for shape, rng in (((64, 64, 128), "native"), ((64, 64, 128), "reference"), ((40, 60, 80), "native")):
        nz = shape[2]
        kw = dict(growth_function=np.exp(-0.4 * np.arange(nz) / nz), mean_matter_density=1.0 + 0.5 * np.arange(nz) / nz, rng=rng, backend="hip")
        a = Generator(*shape, SPACING, **kw)
        a.generate_delta_field(seed=77, save_potential=False)
        want = a.convert_delta_to_density().copy()
        rms = float(a.delta_field_rms)
        a.plan_c2r.device.close()
        b = Generator(*shape, SPACING, **kw)
        got = b.generate_density_field(seed=77)
        assert got.shape == shape and got.dtype == np.float32 and np.all(got > 0)
        assert abs(float(b.delta_field_rms) - rms) <= 1e-6 * rms
        assert np.max(np.abs(got - want) / want) <= 3e-6
        b.plan_c2r.device.close()


@pytest.mark.parametrize("shape", [(64, 64, 64), (256, 256, 256), (128, 64, 512)])
def test_batched_reference_stream_realisations(hip, dpower, shape):
    """rf_realise_batch_reference: n same-seed realisations with the MT19937 replay of seed i + 1 running under the passes of
    seed i (second stream, one set of runs) give, seed by seed, the field of rf_noise_mt19937_ex(single) + rf_realise(RESIDENT)
    -- and that field is the reference's (oracle chain on numpy's own deviates)."""
    k, Pk = dpower
    nx, ny, nz = shape
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    seeds = [123, 7, 2 ** 32 - 1, 5]
    want, rms_want = [], []
    for sd in seeds:
        plan.reference_noise(sd, single=True)
        plan.realise(noise="resident")
        want.append(plan.download_real())
        rms_want.append(plan.moments()[1])
    for n in (1, len(seeds)):
        rms = plan.realise_batch_reference(seeds[:n])
        assert np.array_equal(plan.download_real(), want[n - 1])            # the last seed's field is the current one
        assert np.max(np.abs(rms - np.array(rms_want[:n]))) <= 1e-12 * max(rms_want)
    # every field of a batch, not only the last: batches that END at each seed
    for n in (2, 3):
        plan.realise_batch_reference(seeds[:n], want_rms=False)
        assert np.array_equal(plan.download_real(), want[n - 1])
    ref, rms0 = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, seed=123, double_fft=True)
    assert np.max(np.abs(want[0] - ref)) <= TOL_F32 * rms0
    plan.realise(seed=3)                                                    # (the plan goes back to other work afterwards)
    assert abs(plan.moments()[1] - rms0) < 0.2 * rms0
    plan.close()


def test_merged_yz_launches_give_the_same_field(hip, dpower):
    """rf_k_yz.hip: the z pass of slab s and the y pass of slab s + 1 in one launch (untimed calls by default, timed calls under
    set_merged_yz(2)).  Both halves are the product kernels' own bodies: the field must be bit for bit the one-launch-per-pass
    field, through eager calls, through a graph-replayed batch and with an uploaded k space; rf_merged_yz_ms reports its launches."""
    k, Pk = dpower
    shape = (256, 1024, 1024)                        # 4 slabs of 64 planes
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    assert plan.yz_slabs() == (4, 64)
    plan.set_merged_yz(0)
    plan.realise(seed=77)
    ref = plan.download_real()
    m0 = plan.moments()
    with pytest.raises(RuntimeError):
        plan.merged_yz_ms()                          # no merged launches in that call
    plan.set_merged_yz(2)
    plan.realise(seed=77)
    assert np.array_equal(plan.download_real(), ref) and plan.moments() == m0
    ms, n = plan.merged_yz_ms()
    kern = plan.kernel_ms()
    assert n == 3 and 0.0 < ms < 50.0 and abs(kern[1] - ms) < kern[1] and kern[2] > 0.0
    plan.set_merged_yz(1)                            # the default: timed calls one launch per pass, untimed ones merged
    plan.realise(seed=78)
    other = plan.download_real()
    assert not np.array_equal(other, ref)
    plan.realise_batch(np.array([78, 77], np.uint64), want_rms=False)      # graph replay: merged launches
    assert np.array_equal(plan.download_real(), ref)
    plan.set_merged_yz(0)
    plan.realise_batch(np.array([78], np.uint64), want_rms=False)          # (the captured graphs were dropped with the mode)
    assert np.array_equal(plan.download_real(), other)
    # a slab size that does not divide nx: five slabs of 48 planes and one of 16, merged launches with a smaller last slab
    plan.set_merged_yz(1)
    plan.set_yz_slab_planes(48)
    assert plan.yz_slabs() == (6, 48)
    plan.realise_batch(np.array([78, 77], np.uint64), want_rms=False)
    assert np.array_equal(plan.download_real(), ref) and plan.moments() == m0
    plan.set_merged_yz(2)
    plan.realise(seed=77)
    assert np.array_equal(plan.download_real(), ref) and plan.merged_yz_ms()[1] == 5
    plan.close()
    # a FRESH plan whose first timed call is already merged: rf_kernel_ms must read the merged form's events only (the per-pass
    # event pairs of the one-launch-per-pass form were created for this plan but never recorded)
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    plan.set_merged_yz(2)
    plan.realise(seed=77)
    kern = plan.kernel_ms()
    ms, n = plan.merged_yz_ms()
    assert n == 3 and all(v >= 0.0 for v in kern) and 0.0 < ms <= kern[1] and kern[2] > 0.0
    assert np.array_equal(plan.download_real(), ref)
    plan.set_merged_yz(1)
    plan.realise(seed=77)                            # and back to one launch per pass: the per-pass sums again
    k1 = plan.kernel_ms()
    assert k1[1] > 0.0 and k1[2] > 0.0
    with pytest.raises(RuntimeError):
        plan.merged_yz_ms()
    plan.close()


@pytest.mark.parametrize("shape", [(256, 256, 256), (512, 256, 1024)])
def test_one_call_same_seed_path_equals_the_two_calls(hip, dpower, shape):
    """Generator(rng='reference') on a single-GPU complex64 plan runs replay + passes as ONE device call (rf_realise_batch_reference with
    one seed; rf_can_batch_reference says when).  It must leave the same field, bit for bit, as rf_noise_mt19937_ex(single) followed by
    rf_realise(RESIDENT) -- random.py:24-28 then generate.py:191-199 -- and the same resident deviates for the regenerated potential."""
    from randomfield_amd import Generator
    k, Pk = dpower
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    assert plan.can_batch_reference()
    plan.reference_noise(321, single=True)
    plan.realise(noise="resident")
    two = plan.download_real()
    m_two = plan.moments()
    rms = plan.realise_batch_reference([321], want_rms=True)
    assert np.array_equal(plan.download_real(), two) and abs(rms[0] - m_two[1]) <= 1e-12 * m_two[1]
    assert plan.can_regenerate_potential("resident")
    plan.close()
    assert not hip.DevicePlan(*shape, np.complex128).can_batch_reference()          # (float64 plans: the two calls)
    small = make_plan(hip, (16, 16, 16), np.complex64, k, Pk)
    assert isinstance(small.can_batch_reference(), bool)                             # (tiny grids may or may not have long enough segments)
    small.close()
    nx, ny, nz = shape
    gen = Generator(nx, ny, nz, SPACING, backend="hip")
    d = gen.generate_delta_field(seed=321, save_potential=True)
    assert np.array_equal(d, two) and gen.potential is not None


# ---- the direct exchange: the y pass stores into the peers' receive buffers -------------------------------
def _slab_run_direct(hip, plans, **forward):
    """forward on every (linked) virtual rank -- its y pass stores into the others' receive buffers --, then backward on every rank:
    no exchange step at all"""
    for p in plans:
        p.slab_forward(**forward)
    for p in plans:
        p.slab_backward()
    return np.concatenate([p.download_real() for p in plans], axis=0)


@pytest.mark.parametrize("shape,dtype,nranks,chunks", [((64, 512, 128), np.complex64, 2, 1), ((64, 256, 256), np.complex64, 4, 2), ((64, 64, 512), np.complex64, 8, 1),
                                                       ((32, 16, 128), np.complex128, 2, 2), ((32, 1024, 128), np.complex64, 4, 1), ((16, 2048, 128), np.complex64, 2, 2),
                                                       ((1024, 512, 64), np.complex64, 2, 1), ((16, 1024, 64), np.complex128, 2, 1)])
def test_direct_exchange_between_virtual_ranks_is_bit_identical(hip, dpower, shape, dtype, nranks, chunks):
    """rf_slab_link_direct: the y pass of every virtual rank stores its tiles straight into the receive buffers of the ranks that own
    their x planes (the layout the gathering z pass reads), instead of writing them in place for an all-to-all to move.  Same
    arithmetic per tile, same cells in the same places: the field is that of the copy-exchange path bit for bit -- native generator,
    host deviates through the exact chain, uploaded k space, the fused potential store; whole slabs and sub-slabs; every y-pass
    kernel family (whole-column, two half-length transforms at 1024 and 2048, float64)."""
    k, Pk = dpower
    nx, ny, nz = shape
    plans = _slab_plans(hip, shape, dtype, k, Pk, nranks)
    noise = cpu_ref.reference_noise(5, nx * ny * (nz // 2 + 1))
    for p in plans:
        p.set_exchange_chunks(chunks)
    want = {"native": _slab_run(hip, plans, seed=11), "host noise": _slab_run(hip, plans, noise=noise),
            "potential": _slab_run(hip, plans, seed=11, source="potential")}
    for p in plans:
        p.generate(seed=12)
    want["k space"] = _slab_run(hip, plans, source="kspace")
    stats_want = [p.slab_stats() for p in plans]
    hip.DevicePlan.slab_link_direct(plans)
    got = {"native": _slab_run_direct(hip, plans, seed=11), "host noise": _slab_run_direct(hip, plans, noise=noise),
           "potential": _slab_run_direct(hip, plans, seed=11, source="potential")}
    for p in plans:
        p.generate(seed=12)
    got["k space"] = _slab_run_direct(hip, plans, source="kspace")
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    assert [p.slab_stats() for p in plans] == stats_want
    assert want["native"].std() > 0 and not np.array_equal(want["native"], want["host noise"])
    # linked virtual ranks have no barrier of their own: the whole-call entry points refuse them
    with pytest.raises(RuntimeError):
        plans[0].realise(seed=1)
    # switching the sub-slab count while linked rebuilds the destination table; unlinking restores the copy-exchange path
    if chunks == 1 and shape == (64, 512, 128):
        for p in plans:
            p.set_exchange_chunks(2)
        a = _slab_run_direct(hip, plans, seed=11)
        hip.DevicePlan.slab_link_direct(plans, False)
        assert np.array_equal(_slab_run(hip, plans, seed=11), a)
        for p in plans:
            p.set_exchange_chunks(1)
    hip.DevicePlan.slab_link_direct(plans, False)
    assert np.array_equal(_slab_run(hip, plans, seed=11), want["native"])
    for p in plans:
        p.close()


@pytest.mark.parametrize("shape,kind,chunks", [((64, 512, 128), "c64", 1), ((32, 1024, 256), "c64", 2), ((32, 16, 128), "c128", 1)])
def test_direct_exchange_between_processes_through_ipc_handles(hip, dpower, tmp_path, shape, kind, chunks):
    """The IPC hand-off with REAL processes: two ranks of one job, each a process of its own on this GPU, swap the records of
    rf_slab_direct_export through files, map each other's receive buffers (hipIpcOpenMemHandle) and run the storing y pass into the
    other PROCESS's memory (tests/direct_ipc_worker.py).  The assembled field must be, bit for bit and twice in a row, the field of the
    same two ranks living in one process with the exchange done by device copies.
    (The transport of the records and the barrier are the caller's here; rf_comm_enable_direct does the same over RCCL, which refuses
    two ranks on one device.)"""
    import subprocess
    import sys
    k, Pk = dpower
    nx, ny, nz = shape
    world = 2
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "direct_ipc_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(tmp_path), kind] + [str(v) for v in shape] + [str(chunks)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=400)[0].decode(errors="replace"))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    assert [pr.returncode for pr in procs] == [0] * world, "\n".join(outs)
    assert all((tmp_path / "on_{0}".format(r)).read_bytes() == b"1" for r in range(world))
    got = np.concatenate([np.load(tmp_path / "field_{0}.npy".format(r)) for r in range(world)], axis=1)       # [seed][x][y][z]
    ct = np.complex64 if kind == "c64" else np.complex128
    plans = _slab_plans(hip, shape, ct, k, Pk, world)        # the same two ranks as virtual ranks of THIS process, exchange by device copies
    for p in plans:
        p.set_exchange_chunks(chunks)
    for i, seed in enumerate((11, 12)):
        want = _slab_run(hip, plans, seed=seed)
        assert want.std() > 0 and np.array_equal(got[i], want), (i, seed)
    for p in plans:
        p.close()
    stats = np.sum([np.frombuffer((tmp_path / "stats_{0}".format(r)).read_bytes(), dtype=np.float64) for r in range(world)], axis=0)
    last = got[-1].astype(np.float64)                       # the ranks' local (sum, sum of squares) of the last realisation add up to the field's
    assert abs(stats[0] - last.sum()) <= 1e-6 * np.sqrt(last.size) * last.std() and abs(stats[1] - (last ** 2).sum()) <= 1e-9 * (last ** 2).sum()


def test_direct_exchange_on_one_rank_through_the_whole_call_paths(hip, dpower):
    """rf_comm_enable_direct on a single rank routed through the slab pipeline: rf_realise, rf_realise_potential + the Newtonian
    potential and the pipelined batch run the direct mode's own schedules (storing y pass, barriers, both receive buffers, one and two
    streams, whole slab and sub-slabs) and must give the plain single-GPU plan's fields."""
    k, Pk = dpower
    shape = (256, 128, 256)
    plain = make_plan(hip, shape, np.complex64, k, Pk)
    slab = make_plan(hip, shape, np.complex64, k, Pk)
    with pytest.raises(RuntimeError):
        slab.enable_direct_exchange()                        # neither a communicator nor the forced slab path
    slab.set_force_slab_path(True)
    assert slab.enable_direct_exchange() and slab.direct_exchange_enabled()
    rms_ref = plain.realise_batch([5, 6, 7, 8])
    last = plain.download_real()
    std = plain.moments()[1]
    for chunks in (1, 4, 1):
        slab.set_exchange_chunks(chunks)
        for seed in (3, 4):
            plain.realise(seed=seed)
            slab.realise(seed=seed)
            assert np.max(np.abs(slab.download_real() - plain.download_real())) <= 1e-6 * std
            assert abs(slab.moments()[1] - plain.moments()[1]) <= 1e-6 * std
            assert len(slab.kernel_ms()) == 5
        plain.realise_potential(seed=9)
        slab.realise_potential(seed=9)
        assert np.max(np.abs(slab.download_real() - plain.download_real())) <= 1e-6 * std
        plain.load_potential(-1.5)
        slab.load_potential(-1.5)
        plain.execute_c2r()
        slab.execute_c2r()
        a, b = plain.download_real(), slab.download_real()
        assert np.max(np.abs(a - b)) <= 2e-6 * a.std()
        for n in (1, 2, 4):
            assert np.allclose(slab.realise_batch([5, 6, 7, 8][:n]), rms_ref[:n], rtol=1e-6, atol=0)
        assert np.max(np.abs(slab.download_real() - last)) <= 1e-6 * std
    assert not slab.enable_direct_exchange(False) and not slab.direct_exchange_enabled()
    slab.realise(seed=3)
    plain.realise(seed=3)
    assert np.max(np.abs(slab.download_real() - plain.download_real())) <= 1e-6 * std
    slab.close()
    plain.close()


def test_direct_exchange_refuses_tiles_that_straddle_x_planes(hip, dpower):
    """A y-pass tile has ONE destination only if it lies inside one x plane: kz slabs narrower than the tile keep the copy exchange."""
    k, Pk = dpower
    plans = _slab_plans(hip, (64, 32, 64), np.complex64, k, Pk, 4)          # 8 kz planes per rank, 32-column tiles
    with pytest.raises(RuntimeError):
        hip.DevicePlan.slab_link_direct(plans)
    with pytest.raises(RuntimeError):
        plans[0].set_direct_standin(True)
    ref = _slab_run(hip, plans, seed=2)                                      # ... and still works
    assert np.isfinite(ref).all() and ref.std() > 0
    for p in plans:
        p.close()


def test_direct_standin_runs_the_direct_schedule_on_a_virtual_rank(hip, dpower):
    """rf_slab_set_direct_standin (diagnostics, bench.py's config-4 entry): one rank of a multi-rank plan without a communicator through
    the direct mode's schedules, its stores landing in its own receive buffers.  Not a field (the download refuses); finite,
    reproducible moments; the same moments whether the batch's storing pass runs on the exchange stream or on the plan's."""
    k, Pk = dpower
    shape, P = (256, 64, 256), 4
    plans = _slab_plans(hip, shape, np.complex64, k, Pk, P)
    p = plans[2]
    seen = []
    for overlap in (True, False):
        p.set_direct_standin(True, overlap=overlap)
        p.realise(seed=3)
        m1 = p.moments()
        with pytest.raises(RuntimeError):
            p.download_real()
        rms = p.realise_batch([3, 4, 5])
        p.realise(seed=3)
        assert np.isfinite(m1[1]) and m1[1] > 0 and p.moments() == m1 and np.all(np.isfinite(rms)) and len(rms) == 3
        seen.append(tuple(rms))
    assert seen[0] == seen[1]
    p.set_direct_standin(False)
    with pytest.raises(RuntimeError):
        p.realise(seed=3)                                    # back to "no communicator, no stand-in": loud
    for q in plans:
        q.close()


def _unaligned(shape, rt):
    """a C-contiguous array of that shape that does NOT start on a page boundary"""
    raw = np.empty(int(np.prod(shape)) + 1024 + 16, rt)
    off = ((-raw.ctypes.data) % 4096) // raw.itemsize + 16
    return raw[off:off + int(np.prod(shape))].reshape(shape)


@pytest.mark.parametrize("shape,dtype", [((256, 1024, 1024), np.complex64), ((64, 64, 64), np.complex64), ((128, 512, 1024), np.complex128)])
def test_host_sink_delivers_the_field_slab_by_slab(hip, dpower, shape, dtype):
    """rf_set_host_sink (generate.py:184-189,230: the reference's calls return host arrays): the realisation's own z pass hands every
    finished slab of x planes to a device -> host copy on a second stream.  The host array must be exactly what rf_download_real
    delivers afterwards -- eager native call, the same-seed one-call path, the stored-potential call, float64 (slabs forced by the
    sink) and a grid without slabs -- and the sink is one shot."""
    from randomfield_amd import Generator
    k, Pk = dpower
    plan = make_plan(hip, shape, dtype, k, Pk)
    rt = np.float32 if dtype == np.complex64 else np.float64
    host = np.full(shape[:2] + (shape[2] + 2,), np.nan, rt)
    assert plan.arm_host_sink(host, padded=True)
    plan.realise(seed=5)
    assert plan.host_sink_delivered()
    want = plan.download_real()
    assert np.array_equal(host[:, :, :shape[2]], want) and np.isnan(host[:, :, shape[2]:]).all()
    host[:] = np.nan
    plan.realise(seed=6)                                     # one shot: nothing armed now
    assert not plan.host_sink_delivered() and np.isnan(host).all()
    dense = _unaligned(shape, rt)
    assert plan.arm_host_sink(dense)                         # another buffer, dense rows, any alignment
    plan.realise_potential(seed=7)
    assert plan.host_sink_delivered() and np.array_equal(dense, plan.download_real())
    plan.realise_batch(np.array([8, 9], np.uint64), want_rms=False)        # graph batches are unaffected afterwards
    plan.realise(seed=9)
    ref9 = plan.download_real()
    plan.close()
    if dtype == np.complex64:
        for rng in ("native", "reference"):
            gen = Generator(*shape, SPACING, rng=rng)
            a = gen.generate_delta_field(seed=11, save_potential=False).copy()
            rms_a = gen.delta_field_rms
            assert gen._field_on_host
            gen.generate_delta_field(seed=11, save_potential=False, download=False)
            b = gen.download_field()
            assert np.array_equal(a, b) and gen.delta_field_rms == rms_a and a.std() > 0
            c = gen.generate_delta_field(seed=11, save_potential=True)      # the default call
            assert np.array_equal(c, a)
            gen.plan_c2r.device.close()


def test_failed_realisation_leaves_no_host_sink_armed(hip, monkeypatch):
    """generate_delta_field arms the host sink before the realisation: if that raises (here a Python exception from a replaced
    ``dev.realise``; nothing fails on the GPU), the plan is disarmed again -- the next call that keeps its field on the device
    must not deliver into the old host buffer, and its field is the one a fresh Generator makes, bit for bit."""
    from randomfield_amd import Generator
    shape, seed = (16, 16, 16), 21
    gen = Generator(*shape, SPACING, rng="native")
    dev = gen.plan_c2r.device

    def failing(*args, **kwargs):
        raise RuntimeError("realise failed")
    fresh = Generator(*shape, SPACING, rng="native")
    want = fresh.generate_delta_field(seed=seed, save_potential=False).copy()
    for ask_the_plan in (True, False):          # (asking disarms by itself: the second round leaves that to the Generator alone)
        with monkeypatch.context() as m:
            m.setattr(dev, "realise", failing)
            with pytest.raises(RuntimeError, match="realise failed"):
                gen.generate_delta_field(seed=seed)                      # (download=True: the sink is armed, so the call takes dev.realise)
        if ask_the_plan:
            assert not dev.host_sink_delivered()
        gen.plan_c2r.data_out_padded[...] = np.nan
        assert gen.generate_delta_field(seed=seed, save_potential=False, download=False) is None
        assert not gen._field_on_host and np.isnan(gen.plan_c2r.data_out_padded).all()
        got = gen.download_field()
        assert np.array_equal(got, want) and got.std() > 0
    for g in (gen, fresh):
        g.plan_c2r.device.close()
