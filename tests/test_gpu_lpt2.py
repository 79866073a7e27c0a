"""The second-order (2LPT) displacement on the device (rf_load_hessian, rf_execute_hessian_c2r, rf_lpt2_source, rf_lpt2_potential,
RF_GRAD_FROM_POTENTIAL2; rf_k_misc.hip derivative_kernel / lpt2_accumulate_kernel, rf_k_generic.hip generic_axis_deriv_kernel) and
Generator.calculate_displacement_field(order=2) / lpt2_source -- run with -m gpu on an MI355X.

Oracle: tests/lpt2_oracle.py, float64 numpy, applied to what the device itself holds (the downloaded potential, the downloaded S).
Tolerances: TOL = 1e-5 rms (float32) / 1e-11 rms (float64) per transform, as tests/test_gpu_gradient.py; k space after load_hessian
within 4 eps of the float64 formula with exact zeros where m_a m_b = 0; the source within the per-cell bound
TOL * sum_{a<b} (|H_aa| rms_bb + |H_bb| rms_aa + 2 |H_ab| rms_ab) + 8 eps A(x), A = sum |the six products| (two transformed factors
per product, at most 11 roundings of eps/2 A in the sweep); psi2 against the oracle applied to the device's own S within 2 TOL rms
(two transforms).  Generic plans apply the Hessian factor inside their x pass: that field must be load_hessian + execute_c2r bit for
bit, the four-step fallback of (16384, 4, 6) included.  Shapes: those of tests/test_gpu_gradient.py, one per launch class, its three
nz >= 512 shapes among them ((16, 16, 512) complex64, (8, 8, 512) complex128, (6, 10, 520) complex64: the second kz step of
derivative_kernel, and Hessian, source and second-order potential on the padded potential pitch).  The grid-stride loops of
derivative_kernel and lpt2_accumulate_kernel: tests/test_gpu_at_scale.py."""
import numpy as np
import pytest

import lpt2_oracle as orc
from conftest import golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPACING = 0.5
C64, C128 = np.complex64, np.complex128
TOL = {C64: 1e-5, C128: 1e-11}
TILED = [((16, 16, 16), C64), ((16, 16, 16), C128), ((16, 32, 64), C64),
         ((16, 16, 512), C64), ((8, 8, 512), C128)]     # nz/2 + 1 > 256: two kz steps; float32: potential rows of nz/2 + 64 cells
GENERIC = [((4, 6, 8), C64), ((4, 6, 8), C128), ((40, 60, 80), C64), ((30, 14, 22), C64), ((154, 28, 44), C128), ((2400, 6, 8), C64),
           ((16384, 4, 6), C64), ((6, 10, 520), C64)]       # ... and padded potential rows under the x pass (pitch 324)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else ("c64" if v == C64 else "c128")


def real_of(dtype):
    return np.float32 if dtype == C64 else np.float64


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
    """a random Hermitian half spectrum (as tests/test_gpu_gradient.py)"""
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


def store_potential(plan, delta_k):
    """delta(k) -> the plan's stored potential; returns the device's own copy of it"""
    plan.upload_k(delta_k)
    plan.save_potential()
    plan.load_potential(1.0)
    return plan.download_k().copy()


def assert_elementwise(got, want, factor, dtype):
    eps = np.finfo(real_of(dtype)).eps
    zero = np.broadcast_to(factor == 0, got.shape)
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        err = np.abs(g.astype(np.float64) - w)
        nzw = w != 0
        print("elementwise: max err / (eps |want|) = %.3f" % np.max(err[nzw] / (eps * np.abs(w[nzw]))))
        assert np.all(err <= 4 * eps * np.abs(w))
        assert np.all(g[zero] == 0)


def assert_field(got, oracle, dtype, what, ntransforms=1):
    rms = float(np.std(oracle))
    err = float(np.max(np.abs(got.astype(np.float64) - oracle)))
    print("field %s: max err / rms = %.3g" % (what, err / rms))
    assert rms > 0 and err <= ntransforms * TOL[dtype] * rms


def source_bound(H, dtype, extra_eps=0.0):
    rms = {ab: float(np.std(h)) for ab, h in H.items()}
    lin = sum(np.abs(H[a, a]) * rms[b, b] + np.abs(H[b, b]) * rms[a, a] + 2 * np.abs(H[a, b]) * rms[a, b] for a, b in ((0, 1), (0, 2), (1, 2)))
    return TOL[dtype] * lin + (8 + extra_eps) * np.finfo(real_of(dtype)).eps * orc.source_magnitude(H)


def assert_source(S, H, dtype, what, extra_eps=0.0, want=None):
    want = orc.source_from(H) if want is None else want
    err = np.abs(S.astype(np.float64) - want)
    bound = source_bound(H, dtype, extra_eps)
    print("source %s: max err / bound = %.3g" % (what, np.max(err / bound)))
    assert np.all(bound > 0) and np.all(err <= bound)


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_every_pair_both_sources(hip, shape, dtype):
    plan = make_plan(hip, shape, dtype)
    src = spectrum(shape, dtype)
    pot = store_potential(plan, src)
    dk = orc.dk_of(shape, SPACING)
    scale = 1.5
    for a, b in orc.PAIRS:
        factor = orc.hessian_factor(shape, SPACING, a, b, scale)
        for source, data in ((hip.RF_GRAD_FROM_KSPACE, src), (hip.RF_GRAD_FROM_POTENTIAL, pot)):
            divide = source == hip.RF_GRAD_FROM_KSPACE
            want = orc.hessian_k(data, shape, SPACING, a, b, scale, divide)
            plan.upload_k(src)
            plan.load_hessian(a, b, scale, dk[a], dk[b], source)
            assert_elementwise(plan.download_k(), want, factor, dtype)
            plan.execute_c2r()
            two_steps = plan.download_real().copy()
            plan.upload_k(src)
            plan.execute_hessian(a, b, scale, dk[a], dk[b], source)
            got = plan.download_real()
            assert_field(got, orc.irfftn(want, shape), dtype, "H_%d%d source %d" % (a, b, source))
            if not plan.tiled:           # the factor inside the x pass (or the fallback into scratch): same values through the same stages
                assert np.array_equal(got, two_steps)
            assert abs(plan.moments()[1] - got.astype(np.float64).std()) <= 1e-5 * got.std()
            if divide:                   # delta(k) was consumed, as by the gradient
                with pytest.raises(RuntimeError, match="no k-space data"):
                    plan.download_k()
    if shape[0] == 16384:                # the x axis in the four-step form: the elementwise sweep is a launch of its own
        assert plan.kernel_ms()[4] > 0
    plan.load_potential(1.0)             # the stored potential was only read
    assert np.array_equal(plan.download_k(), pot)
    plan.close()


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_source_and_second_order_displacement(hip, shape, dtype):
    plan = make_plan(hip, shape, dtype)
    src = spectrum(shape, dtype)
    pot = store_potential(plan, src)
    dk = orc.dk_of(shape, SPACING)
    before = plan.nbytes
    plan.execute_gradient(1, 1.0, dk[1], hip.RF_GRAD_FROM_POTENTIAL)
    first_order = plan.download_real().copy()
    # nothing to read yet: refused, and nothing queued
    plan.upload_k(src)
    for call in (plan.load_gradient, plan.execute_gradient):
        with pytest.raises(RuntimeError, match="no second-order potential"):
            call(0, 1.0, dk[0], hip.RF_GRAD_FROM_POTENTIAL2)
    assert np.array_equal(plan.download_k(), src) and np.array_equal(plan.download_real(), first_order)

    plan.lpt2_source(dk)
    S = plan.download_real().copy()
    H = orc.hessian_fields(pot, shape, SPACING)
    assert_source(S, H, dtype, "of the stored potential")
    assert abs(float(S.astype(np.float64).mean())) <= TOL[dtype] * float(np.std(S))
    assert plan.nbytes >= before + 2 * S.nbytes                 # the accumulators are counted
    with pytest.raises(RuntimeError, match="no k-space data"):
        plan.download_k()
    with pytest.raises(RuntimeError, match="no realisation"):
        plan.moments()
    plan.lpt2_source(dk)
    assert np.array_equal(plan.download_real(), S)              # the same bits on every call
    with pytest.raises(RuntimeError, match="no second-order potential"):
        plan.execute_gradient(0, 1.0, dk[0], hip.RF_GRAD_FROM_POTENTIAL2)

    plan.lpt2_potential(dk)
    Sk = plan.download_k()                                      # K holds S(k)
    want_k = orc.rfftn(S)
    assert np.max(np.abs(Sk - want_k)) <= TOL[dtype] * float(np.sqrt(np.mean(np.abs(want_k) ** 2)))
    for axis in range(3):
        plan.execute_gradient(axis, 3.0 / 7.0, dk[axis], hip.RF_GRAD_FROM_POTENTIAL2)
        assert_field(plan.download_real(), orc.displacement2_from_source(S, shape, SPACING, axis), dtype, "psi2 axis %d" % axis, 2)
    plan.load_gradient(2, 3.0 / 7.0, dk[2], hip.RF_GRAD_FROM_POTENTIAL2)
    plan.execute_c2r()
    if not plan.tiled:
        plan.execute_gradient(2, 3.0 / 7.0, dk[2], hip.RF_GRAD_FROM_POTENTIAL2)
        fused = plan.download_real().copy()
        plan.load_gradient(2, 3.0 / 7.0, dk[2], hip.RF_GRAD_FROM_POTENTIAL2)
        plan.execute_c2r()
        assert np.array_equal(plan.download_real(), fused)

    # the stored potential and its first-order gradient are what they were
    plan.execute_gradient(1, 1.0, dk[1], hip.RF_GRAD_FROM_POTENTIAL)
    assert np.array_equal(plan.download_real(), first_order)
    plan.load_potential(1.0)
    assert np.array_equal(plan.download_k(), pot)
    # a new stored potential drops the second-order one
    plan.upload_k(src)
    plan.save_potential()
    with pytest.raises(RuntimeError, match="no second-order potential"):
        plan.execute_gradient(0, 1.0, dk[0], hip.RF_GRAD_FROM_POTENTIAL2)
    assert np.array_equal(plan.download_k(), src)
    plan.close()


def test_realise_potential_drops_the_second_order_potential(hip, dpower):
    shape, dtype = (16, 16, 16), C64
    plan = make_plan(hip, shape, dtype, dpower)
    dk = orc.dk_of(shape, SPACING)
    plan.realise_potential(seed=21)
    plan.lpt2_potential(dk)
    plan.execute_gradient(0, 3.0 / 7.0, dk[0], hip.RF_GRAD_FROM_POTENTIAL2)
    a = plan.download_real().copy()
    plan.realise_potential(seed=22)
    field = plan.download_real().copy()
    with pytest.raises(RuntimeError, match="no second-order potential"):
        plan.execute_gradient(0, 3.0 / 7.0, dk[0], hip.RF_GRAD_FROM_POTENTIAL2)
    assert np.array_equal(plan.download_real(), field)          # nothing was queued
    plan.lpt2_potential(dk)
    plan.execute_gradient(0, 3.0 / 7.0, dk[0], hip.RF_GRAD_FROM_POTENTIAL2)
    assert not np.array_equal(plan.download_real(), a)
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((16, 16, 16), C64), ((16, 16, 16), C128), ((40, 60, 80), C64)], ids=_ids)
def test_two_wave_closed_form_through_an_uploaded_potential(hip, shape, dtype):
    """phi = A cos(k1 x) + B cos(k2 y) uploaded as delta = k^2 phi and stored.  Besides the source's own bound: the upload rounds every
    mode of delta, and rf_save_potential rounds k^2 twice, 1 / k^2 and the product -- under 2 eps per mode; every H component is one
    mode here, so every product moves by under 4 eps of itself: 4 eps A(x) more."""
    plan = make_plan(hip, shape, dtype)
    phi, closed = orc.two_wave_potential(shape, SPACING, 1.5, -0.7, 2, 3, 0.3, 0.5)
    store_potential(plan, (phi * orc.ksq_grid(shape, SPACING)).astype(dtype))
    plan.lpt2_source(orc.dk_of(shape, SPACING))
    H = orc.hessian_fields(phi, shape, SPACING)
    assert_source(plan.download_real(), H, dtype, "two waves", extra_eps=4.0, want=closed)
    plan.close()


def check_generator(gen, shape, dtype):
    """the three order=2 components and the source against the oracle on the generator's own potential; returns the components"""
    from randomfield_amd.generate import _DevicePotential
    comps = [gen.calculate_displacement_field(axis, order=2).copy() for axis in range(3)]
    assert isinstance(gen.potential, _DevicePotential)
    pot = gen.potential.download().astype(C128)
    assert [np.array_equal(gen.calculate_displacement_field(a, order=2), comps[a]) for a in range(3)] == [True] * 3   # (reading P disturbed nothing)
    S = gen.lpt2_source().copy()
    assert_source(S, orc.hessian_fields(pot, shape, SPACING), dtype, "generator")
    for axis, name in enumerate("xyz"):
        assert_field(comps[axis], orc.displacement2_from_source(S, shape, SPACING, axis), dtype, "generator psi2 %s" % name, 2)
        assert np.array_equal(gen.calculate_displacement_field(name, order=2), comps[axis])      # (rebuilt after lpt2_source: same bits)
    return comps


def test_generator_regenerated_and_stored_potential(hip):
    from randomfield_amd import Generator
    from randomfield_amd.generate import _DevicePotential, _RegeneratedPotential
    shape, dtype = (16, 16, 16), C64
    regen = Generator(*shape, SPACING, rng="native")
    stored = Generator(*shape, SPACING, rng="native", store_potential=True)
    for gen in (regen, stored):
        gen.generate_delta_field(seed=1234, save_potential=True, download=False)
    assert isinstance(regen.potential, _RegeneratedPotential) and isinstance(stored.potential, _DevicePotential)
    rms = stored.delta_field_rms
    order1 = [stored.calculate_displacement_field(a).copy() for a in range(3)]
    a = check_generator(stored, shape, dtype)
    b = check_generator(regen, shape, dtype)
    for axis in range(3):                       # the same field from the same seed: the two routes agree as two transforms do
        assert_field(b[axis], a[axis].astype(np.float64), dtype, "regenerated against stored %d" % axis, 2)
        assert np.array_equal(stored.calculate_displacement_field(axis), order1[axis])         # order 1 before and after: the same bits
    assert stored.delta_field_rms == rms
    fz = 1.0 / (1.0 + 0.1 * np.arange(shape[2]))
    scaled = stored.calculate_displacement_field(0, order=2, scale=2.0, factor_z=fz).copy()
    assert np.max(np.abs(scaled - 4.0 * a[0] * fz)) <= 2 * TOL[dtype] * 4.0 * float(np.std(a[0]))
    # a new realisation drops the cached second-order potential
    stored.generate_delta_field(seed=99, save_potential=True, download=False)
    c = check_generator(stored, shape, dtype)
    assert not np.array_equal(c[0], a[0])
    with pytest.raises(ValueError, match="order"):
        stored.calculate_displacement_field(0, order=3)
    with pytest.raises(RuntimeError, match="No saved potential field."):
        Generator(*shape, SPACING, rng="native").calculate_displacement_field(0, order=2)


def test_generator_generic_shape(hip):
    from randomfield_amd import Generator
    shape = (40, 60, 80)                        # (the Generator wants nz a multiple of 4)
    gen = Generator(*shape, SPACING, rng="native", store_potential=True)
    gen.generate_delta_field(seed=7, save_potential=True, download=False)
    check_generator(gen, shape, C64)


def test_refusals_leave_the_plan_usable(hip):
    shape = (16, 16, 16)
    plan = make_plan(hip, shape, C64)
    src = spectrum(shape, C64)
    dk = orc.dk_of(shape, SPACING)
    plan.upload_k(src)
    K, P = hip.RF_GRAD_FROM_KSPACE, hip.RF_GRAD_FROM_POTENTIAL
    for call in (plan.load_hessian, plan.execute_hessian):
        with pytest.raises(RuntimeError, match="axes"):
            call(0, 3, 1.0, dk[0], dk[0], K)
        with pytest.raises(RuntimeError, match="axes"):
            call(-1, 1, 1.0, dk[0], dk[0], K)
        with pytest.raises(RuntimeError, match="a <= b"):
            call(2, 1, 1.0, dk[2], dk[1], K)
        with pytest.raises(RuntimeError, match="no saved potential"):
            call(0, 1, 1.0, dk[0], dk[1], P)
        with pytest.raises(RuntimeError, match="source"):
            call(0, 1, 1.0, dk[0], dk[1], hip.RF_GRAD_FROM_POTENTIAL2)
    for call in (plan.lpt2_source, plan.lpt2_potential):
        with pytest.raises(RuntimeError, match="no saved potential"):
            call(dk)
    assert np.array_equal(plan.download_k(), src)             # nothing was queued
    plan.execute_hessian(0, 1, 1.0, dk[0], dk[1], K)
    assert_field(plan.download_real(), orc.irfftn(orc.hessian_k(src, shape, SPACING, 0, 1, 1.0, True), shape), C64, "after the refusals")
    plan.close()
    c2c = hip.DevicePlan(16, 16, 16, C64, unpacked=True)
    for call in (c2c.load_hessian, c2c.execute_hessian):
        with pytest.raises(RuntimeError, match="c2c"):
            call(0, 1, 1.0, 1.0, 1.0, K)
    for call in (c2c.lpt2_source, c2c.lpt2_potential):
        with pytest.raises(RuntimeError, match="c2c"):
            call(dk)
    data = (np.arange(16 ** 3) % 7).astype(C64).reshape(shape)
    c2c.upload_c(data)
    c2c.execute_c2c(inverse=False)
    assert np.allclose(c2c.download_c(), np.fft.fftn(data), atol=1e-2)      # still works
    c2c.close()
