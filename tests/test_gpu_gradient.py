"""The gradient of the saved potential on the device (rf_load_gradient, rf_execute_gradient_c2r; rf_k_misc.hip derivative_kernel,
rf_k_generic.hip generic_axis_deriv_kernel) and Generator.calculate_displacement_field -- run with -m gpu on an MI355X.

Oracle: numpy in float64, np.fft.irfftn(1j * k_a * Phat) with the axis' Nyquist entry of k_a set to 0, Phat being the k space the
device itself holds (download_k) or the uploaded array.  Tolerances: k space after load_gradient within 4 eps per component of the
float64 formula on the same input (two roundings, the factor and the product: ~1 eps; 4 is the margin) with exact zeros where the
rule says zero; fields within 1e-5 * rms (float32) / 1e-11 * rms (float64) on the maximum absolute error, as tests/test_gpu_generic.py.
Generic plans apply the factor inside their x pass: that field must be load_gradient + execute_c2r bit for bit.

Shapes: tiled plans (16, 16, 16) both dtypes and (16, 32, 64); generic plans one workgroup (4, 6, 8), tile 16 in place (40, 60, 80), a
ragged last workgroup (30, 14, 22), two LDS buffers (154, 28, 44), tile 4 (2400, 6, 8), and an x axis in the four-step form
(16384, 4, 6), which takes the elementwise kernel into scratch.  nz >= 512 -- rows of nz/2 + 1 > 256 cells, so the kernels' kz loop
takes a second step, and on float32 plans potential rows padded to nz/2 + 64 cells: tiled (16, 16, 512) complex64 (pitch 320; also
under test_stored_potential, where the generation pass itself writes the potential) and (8, 8, 512) complex128 (no padding), generic
(6, 10, 520) complex64 (pitch 324 read by the x pass).  More rows or cells than one launch holds: tests/test_gpu_at_scale.py."""
import numpy as np
import pytest

from conftest import golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPACING = 0.5
C64, C128 = np.complex64, np.complex128
TOL = {C64: 1e-5, C128: 1e-11}
TILED = [((16, 16, 16), C64), ((16, 16, 16), C128), ((16, 32, 64), C64),
         ((16, 16, 512), C64), ((8, 8, 512), C128)]     # nz/2 + 1 > 256: two kz steps; float32: potential rows of nz/2 + 64 cells
GENERIC = [((4, 6, 8), C64), ((4, 6, 8), C128), ((40, 60, 80), C64), ((30, 14, 22), C64), ((154, 28, 44), C128), ((2400, 6, 8), C64),
           ((6, 10, 520), C64)]       # the x pass reads padded potential rows (pitch 324)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else ("c64" if v == C64 else "c128")


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def dpower():
    d = golden("default_power.npz")
    return d["k"], d["Pk"]


def make_plan(hip, shape, dtype, power=None):
    from randomfield_amd import powertools
    nx, ny, nz = shape
    plan = hip.DevicePlan(nx, ny, nz, dtype)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    if power is not None:
        xt, st = cpu_ref.sigma_table(power[0], power[1], nx, ny, nz, SPACING)
        plan.set_power(xt, st)
    return plan


def spectrum(shape, dtype, seed=5):
    """a random Hermitian half spectrum: symmetrised as the generator's where transform.symmetrize takes the shape (an odd number of
    stored planes), else by averaging the kz = 0 and nz/2 planes with their mirrored conjugates"""
    from randomfield_amd import transform
    nx, ny, nz = shape
    rng = np.random.RandomState(seed)
    data = (rng.normal(size=(nx, ny, nz // 2 + 1)) + 1j * rng.normal(size=(nx, ny, nz // 2 + 1))).astype(dtype)
    if (nz // 2 + 1) % 2:
        transform.symmetrize(data, packed=True)
    else:
        for kz in (0, nz // 2):
            plane = data[:, :, kz]
            data[:, :, kz] = 0.5 * (plane + np.conj(np.roll(plane[::-1, ::-1], (1, 1), axis=(0, 1))))
        data[0, 0, 0] = 0
    return data


def dk_of(shape, axis):
    return 2 * np.pi / (shape[axis] * SPACING)


def k_axis(shape, axis):
    n = shape[axis]
    k = 2 * np.pi * (np.fft.rfftfreq(n, SPACING) if axis == 2 else np.fft.fftfreq(n, SPACING))
    k[n // 2] = 0.0
    return k.reshape([-1 if a == axis else 1 for a in range(3)])


def want_k(src, shape, axis, scale, divide):
    """the float64 formula on the same input (divide: the source is delta(k); k^2 from the plan's own tables)"""
    from randomfield_amd import powertools
    out = 1j * scale * k_axis(shape, axis) * src.astype(C128)
    if divide:
        kx2, ky2, kz2 = (np.asarray(a, np.float64) for a in powertools.ksq_axes(*shape, SPACING))
        k2 = (kx2[:, None, None] + ky2[None, :, None]) + kz2[None, None, :]
        k2[0, 0, 0] = 1.0
        out = out / k2
        out[0, 0, 0] = 0.0
    return out


def assert_elementwise(got, want, dtype):
    eps = np.finfo(np.float32 if dtype == C64 else np.float64).eps
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        err = np.abs(g.astype(np.float64) - w)
        nz = w != 0
        print("elementwise: max err / (eps |want|) = %.3f" % np.max(err[nz] / (eps * np.abs(w[nz]))))
        assert np.all(err <= 4 * eps * np.abs(w))
        assert np.all(g[~nz] == 0)


def assert_field(got, oracle, dtype, what):
    rms = float(np.std(oracle))
    err = float(np.max(np.abs(got.astype(np.float64) - oracle)))
    print("field %s: max err / rms = %.3g" % (what, err / rms))
    assert rms > 0 and err <= TOL[dtype] * rms


def irfftn(k, shape):
    return np.fft.irfftn(k, s=shape, axes=(0, 1, 2))


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_uploaded_spectrum_every_axis(hip, shape, dtype):
    plan = make_plan(hip, shape, dtype)
    src = spectrum(shape, dtype)
    K, scale = hip.RF_GRAD_FROM_KSPACE, 1.5
    for axis in range(3):
        want = want_k(src, shape, axis, scale, True)
        plan.upload_k(src)
        plan.load_gradient(axis, scale, dk_of(shape, axis), K)
        assert_elementwise(plan.download_k(), want, dtype)
        plan.execute_c2r()
        two_steps = plan.download_real().copy()
        plan.upload_k(src)
        plan.execute_gradient(axis, scale, dk_of(shape, axis), K)
        got = plan.download_real()
        assert_field(got, irfftn(want, shape), dtype, "axis %d" % axis)
        if not plan.tiled:           # the factor inside the x pass: same values, same LDS positions, same stages
            assert np.array_equal(got, two_steps)
        assert abs(plan.moments()[1] - got.astype(np.float64).std()) <= 1e-5 * got.std()
    plan.close()


def test_four_step_x_axis_takes_the_fallback(hip):
    shape, dtype = (16384, 4, 6), C64
    plan = make_plan(hip, shape, dtype)
    src = spectrum(shape, dtype)
    for axis in (0, 2):
        plan.upload_k(src)
        plan.execute_gradient(axis, 1.0, dk_of(shape, axis), hip.RF_GRAD_FROM_KSPACE)
        assert_field(plan.download_real(), irfftn(want_k(src, shape, axis, 1.0, True), shape), dtype, "axis %d" % axis)
        assert plan.kernel_ms()[4] > 0                        # the elementwise sweep is reported as a launch of its own
    plan.close()
    plan = make_plan(hip, (40, 60, 80), dtype)                # ... and there is none where the x pass applies the factor
    plan.upload_k(spectrum((40, 60, 80), dtype))
    plan.execute_gradient(0, 1.0, dk_of((40, 60, 80), 0), hip.RF_GRAD_FROM_KSPACE)
    ms = plan.kernel_ms()
    assert ms[4] == 0 and ms[0] > 0
    plan.close()


@pytest.mark.parametrize("shape", [(16, 16, 16), (40, 60, 80), (16, 16, 512)], ids=_ids)
def test_stored_potential(hip, dpower, shape):
    dtype = C64
    plan = make_plan(hip, shape, dtype, dpower)
    plan.realise_potential(seed=21)
    plan.load_potential(1.0)
    pot = plan.download_k().copy()
    P, scale = hip.RF_GRAD_FROM_POTENTIAL, -0.75
    for axis in range(3):
        plan.load_gradient(axis, scale, dk_of(shape, axis), P)
        assert_elementwise(plan.download_k(), want_k(pot, shape, axis, scale, False), dtype)
        plan.realise(seed=4)                                  # (something else in the field buffer)
        plan.execute_gradient(axis, scale, dk_of(shape, axis), P)
        assert_field(plan.download_real(), irfftn(want_k(pot, shape, axis, scale, False), shape), dtype, "axis %d" % axis)
    plan.load_potential(1.0)                                  # the stored potential is only read
    assert np.array_equal(plan.download_k(), pot)
    plan.close()


def test_generator_regenerated_and_stored_potential_agree(hip, dpower):
    from randomfield_amd import Generator
    from randomfield_amd.generate import _DevicePotential, _RegeneratedPotential
    shape = (16, 16, 16)
    fz = 1.0 / (1.0 + 0.1 * np.arange(shape[2]))
    regen = Generator(*shape, SPACING, rng="native")
    stored = Generator(*shape, SPACING, rng="native", store_potential=True)
    for gen in (regen, stored):
        gen.generate_delta_field(seed=1234, save_potential=True, download=False)
    assert isinstance(regen.potential, _RegeneratedPotential) and isinstance(stored.potential, _DevicePotential)
    rms = stored.delta_field_rms
    pot = stored.potential.download().astype(C128)
    for axis, name in enumerate("xyz"):
        want = stored.calculate_displacement_field(axis).copy()
        assert_field(want, irfftn(want_k(pot, shape, axis, 1.0, False), shape), C64, "stored %s" % name)
        got = regen.calculate_displacement_field(name).copy()
        assert_field(got, want.astype(np.float64), C64, "regenerated against stored %s" % name)
        scaled = stored.calculate_displacement_field(axis, scale=2.0, factor_z=fz).copy()
        assert np.max(np.abs(scaled - 2.0 * want * fz)) <= 2e-6 * 2.0 * float(np.std(want))
    assert stored.delta_field_rms == rms and isinstance(stored.potential, _DevicePotential)
    with pytest.raises(RuntimeError, match="No saved potential field."):
        Generator(*shape, SPACING, rng="native").calculate_displacement_field(0)


def test_generator_default_rng_regenerated_against_stored(hip):
    """The constructor's defaults (rng='reference', complex64): the replayed stream is resident as float32 pairs and the potential is
    not stored.  The first component runs the storing form of the realisation once; all three must agree with
    Generator(store_potential=True) for the same seed at the field tolerance, and with the float64 oracle on the stored potential."""
    from randomfield_amd import Generator
    from randomfield_amd.generate import _DevicePotential, _RegeneratedPotential
    shape = (16, 16, 16)
    regen = Generator(*shape, SPACING)
    stored = Generator(*shape, SPACING, store_potential=True)
    for gen in (regen, stored):
        gen.generate_delta_field(seed=77, save_potential=True, download=False)
    assert isinstance(regen.potential, _RegeneratedPotential) and regen.potential.noise == "resident"
    assert isinstance(stored.potential, _DevicePotential)
    rms = regen.delta_field_rms
    pot = stored.potential.download().astype(C128)
    for axis, name in enumerate("xyz"):
        want = stored.calculate_displacement_field(axis).copy()
        assert_field(want, irfftn(want_k(pot, shape, axis, 1.0, False), shape), C64, "reference stream, stored %s" % name)
        got = regen.calculate_displacement_field(name).copy()
        assert_field(got, want.astype(np.float64), C64, "reference stream, regenerated against stored %s" % name)
    assert regen.delta_field_rms == rms
    # the Newtonian potential of the same object still works afterwards, and is the stored route's
    a = regen.calculate_newtonian_potential(light_cone=False, scale=-2.5e-3).copy()
    b = stored.calculate_newtonian_potential(light_cone=False, scale=-2.5e-3).copy()
    assert_field(a, b.astype(np.float64), C64, "newtonian potential afterwards")


def test_refusals_leave_the_plan_usable(hip):
    shape = (16, 16, 16)
    plan = make_plan(hip, shape, C64)
    src = spectrum(shape, C64)
    plan.upload_k(src)
    K, P = hip.RF_GRAD_FROM_KSPACE, hip.RF_GRAD_FROM_POTENTIAL
    for call in (plan.load_gradient, plan.execute_gradient):
        with pytest.raises(RuntimeError, match="axis"):
            call(3, 1.0, dk_of(shape, 0), K)
        with pytest.raises(RuntimeError, match="no saved potential"):
            call(0, 1.0, dk_of(shape, 0), P)
        with pytest.raises(RuntimeError, match="source"):
            call(0, 1.0, dk_of(shape, 0), 7)
    assert np.array_equal(plan.download_k(), src)             # nothing was queued
    plan.execute_gradient(1, 1.0, dk_of(shape, 1), K)
    assert_field(plan.download_real(), irfftn(want_k(src, shape, 1, 1.0, True), shape), C64, "after the refusals")
    with pytest.raises(RuntimeError, match="no k-space data"):     # FROM_KSPACE consumed the k buffer
        plan.execute_gradient(1, 1.0, dk_of(shape, 1), K)
    plan.close()
    c2c = hip.DevicePlan(16, 16, 16, C64, unpacked=True)
    for call in (c2c.load_gradient, c2c.execute_gradient):
        with pytest.raises(RuntimeError, match="c2c"):
            call(0, 1.0, 1.0, K)
    data = (np.arange(16 ** 3) % 7).astype(C64).reshape(shape)
    c2c.upload_c(data)
    c2c.execute_c2c(inverse=False)
    assert np.allclose(c2c.download_c(), np.fft.fftn(data), atol=1e-2)      # still works
    c2c.close()
