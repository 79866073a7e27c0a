"""The cloud-in-cell gather on the device (rf_particles_gather / _gather_download / _shift, the diagnostic rf_particles_set_gather_form;
rf_k_particles.hip cic_gather_global_kernel / cic_gather_tiled_kernel) and Generator.interpolate_at_particles / shift_particles -- run
with -m gpu on an MI355X.

Oracle: tests/gather_oracle.py applied to the very arrays that were uploaded.  The definition fixes every rounding (float64 products
and sums, each rounded on its own, one rounding to the plan's real type), so every form -- loads from memory, LDS tiles, the library's
choice -- must give the oracle's values with np.array_equal.  The shift is the accumulate step: one fma rounding, held to the
two-rounding bound 2 eps (|Q| + |coeff G|) of tests/test_gpu_particles.py.

Shapes: tiled plans (16, 16, 16) both dtypes and (16, 32, 64); generic plans (4, 6, 8) both dtypes, (30, 14, 22) and (40, 60, 80); and
one case of (130, 126, 66) = 1 081 080 particles: form 1's grid is capped at 4096 workgroups of 256 lanes = 1 048 576, so its second
stride runs and ends in a partial wave (32 504 = 507 x 64 + 56), and form 2's bricks (8, 8, 64) are partial on all three axes."""
import numpy as np
import pytest

import cic_oracle as orc
import gather_oracle as gorc

pytestmark = pytest.mark.gpu

SPACING = 0.5            # a power of two: whole and half cells are exact in float32
INV_H = [1.0 / SPACING] * 3
C64, C128 = np.complex64, np.complex128
TILED = [((16, 16, 16), C64), ((16, 16, 16), C128), ((16, 32, 64), C64)]
GENERIC = [((4, 6, 8), C64), ((4, 6, 8), C128), ((30, 14, 22), C64), ((40, 60, 80), C64)]
FORMS = (1, 2, 0)
COEFF = 0.3              # not a power of two: the coefficient stays float64 inside the gather


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else ("c64" if v == C64 else "c128")


def real_of(dtype):
    return np.float32 if dtype == C64 else np.float64


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def upload(plan, s3):
    for a in range(3):
        plan.particles_upload(a, np.ascontiguousarray(s3[a]))


def gather_all_forms(plan, s, W, what, wdrop=0):
    """`first` into slot 0 and an add with COEFF onto it, under both forced forms and the library's choice: equal to the oracle"""
    want, drop = gorc.gather(s, INV_H, W)
    want_add, _ = gorc.gather(s, INV_H, W, COEFF, False, want)
    assert drop == wdrop
    for form in FORMS:
        plan.set_gather_form(form)
        slot = form                                                # (every slot is used)
        assert plan.particles_gather(INV_H, slot, 1.0, True) == wdrop, (what, form)
        assert np.array_equal(plan.particles_gather_download(slot), want, equal_nan=True), (what, form)
        assert plan.particles_gather(INV_H, slot, COEFF, False) == wdrop, (what, form)
        assert np.array_equal(plan.particles_gather_download(slot), want_add, equal_nan=True), (what, form)
    plan.set_gather_form(0)
    return want


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_gather_every_set_every_form(hip, shape, dtype):
    rt = real_of(dtype)
    rng = np.random.RandomState(sum(shape))
    W = rng.normal(size=shape).astype(rt)
    Wint = rng.randint(-15, 16, size=shape).astype(rt)
    plan = hip.DevicePlan(*shape, dtype)
    sets = {name: s.astype(rt) for name, s in orc.displacement_sets(shape, SPACING).items()}
    for name, s in sets.items():
        upload(plan, s)
        plan.upload_real(W)
        got = gather_all_forms(plan, s, W, name)
        if name == "zero":
            assert np.array_equal(got, W)
        if name == "plus3":
            assert np.array_equal(got, np.roll(W, (-3, -3, -3), (0, 1, 2)))
        # the adjoint identity against the paint of the same Q: sum_q g 2^48 == sum_cells A W, in integers (|W| <= 15: every step exact;
        # g comes back exactly in float32 too only where it has 24 bits, so the identity is checked on float64 plans and, for float32,
        # through the oracle's exact g of the same uploaded arrays)
        plan.upload_real(Wint)
        plan.particles_gather(INV_H, 0, 1.0, True)
        G = plan.particles_gather_download(0)
        plan.particles_paint(INV_H)
        A = plan.particles_download_counts()
        rhs = sum(int(a) * int(w) for a, w in zip(A.ravel(), Wint.ravel()))
        g, _ = gorc.gather_g(s, INV_H, Wint)
        assert np.array_equal(G, g.astype(rt)), name
        scaled = (G.astype(np.float64) if rt == np.float64 else g) * 2.0 ** 48
        assert np.all(scaled == np.floor(scaled)) and sum(int(v) for v in scaled.ravel()) == rhs, name
    # one NaN and one +inf planted in the random set: counted, `first` writes 0, an add leaves G
    s = sets["rms3"].copy()
    p1, p2 = (1, 2, 3), tuple(m - 1 for m in shape)
    s[1][p1] = np.nan
    s[2][p2] = np.inf
    upload(plan, s)
    plan.upload_real(W)
    got = gather_all_forms(plan, s, W, "non-finite", wdrop=2)
    assert got[p1] == 0 and got[p2] == 0
    # a non-finite field value reaches the particles around it
    Wn = W.copy()
    Wn[p1] = np.nan
    upload(plan, sets["small"])
    plan.upload_real(Wn)
    got = gather_all_forms(plan, sets["small"], Wn, "nan field")
    assert 1 <= np.count_nonzero(np.isnan(got)) <= 27
    plan.close()


def test_second_stride_partial_wave_and_partial_bricks(hip):
    shape, rt = (130, 126, 66), np.float32
    assert int(np.prod(shape)) == 1081080 > 4096 * 256 and (1081080 - 4096 * 256) % 64 == 56
    assert all(n % b for n, b in zip(shape, (8, 8, 64)))
    rng = np.random.RandomState(7)
    W = rng.normal(size=shape).astype(rt)
    s = (rng.normal(scale=1.5, size=(3,) + shape) * SPACING).astype(rt)
    s[0][129, 125, 65] = np.nan                                    # the last particle: the partial wave of the second stride
    want, wdrop = gorc.gather(s, INV_H, W)
    want_add, _ = gorc.gather(s, INV_H, W, COEFF, False, want)
    assert wdrop == 1
    plan = hip.DevicePlan(*shape, C64)
    upload(plan, s)
    plan.upload_real(W)
    for form in FORMS:
        plan.set_gather_form(form)
        assert plan.particles_gather(INV_H, 1, 1.0, True) == 1
        assert np.array_equal(plan.particles_gather_download(1), want), form
        assert plan.particles_gather(INV_H, 1, COEFF, False) == 1
        assert np.array_equal(plan.particles_gather_download(1), want_add), form
    plan.close()


def test_nothing_but_the_slot_changes(hip):
    from randomfield_amd import powertools
    shape, dtype, rt = (16, 16, 16), C64, np.float32
    plan = hip.DevicePlan(*shape, dtype)
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    rng = np.random.RandomState(5)
    src = (rng.normal(size=plan.k_shape) + 1j * rng.normal(size=plan.k_shape)).astype(dtype)
    plan.upload_k(src)
    plan.save_potential()
    plan.load_potential(1.0)
    pot = plan.download_k().copy()
    plan.upload_k(src)
    s = orc.displacement_sets(shape, SPACING)["rms3"].astype(rt)
    upload(plan, s)
    plan.particles_paint(INV_H)
    before = plan.nbytes

    def state():
        return [plan.download_real().copy()] + [plan.particles_download(a).copy() for a in range(3)] + [plan.particles_download_counts().copy(),
                                                                                                       plan.download_k().copy()]

    was = state()
    with pytest.raises(RuntimeError, match="no gathered values"):
        plan.particles_gather_download(0)
    with pytest.raises(RuntimeError, match="no gathered values"):
        plan.particles_shift(0, 0, 1.0)
    assert plan.nbytes == before
    for form in FORMS:
        plan.set_gather_form(form)
        plan.particles_gather(INV_H, 2, 1.0, True)
        plan.particles_gather(INV_H, 2, COEFF, False)
        assert plan.nbytes == before + 3 * was[0].nbytes           # G: three arrays of the field's size, allocated once
        for a, b in zip(was, state()):
            assert np.array_equal(a, b), form
    assert not plan.particles_gather_download(0).any() and not plan.particles_gather_download(1).any()      # (allocated zeroed)
    assert np.array_equal(plan.particles_gather_download(2), gorc.gather(s, INV_H, was[0], COEFF, False, gorc.gather(s, INV_H, was[0])[0])[0])
    ms = plan.kernel_ms()                                          # the gather alone
    assert len(ms) == 5 and ms[0] > 0 and ms[4] == 0
    assert plan.elapsed_ms() > 0
    plan.load_potential(1.0)
    assert np.array_equal(plan.download_k(), pot)
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((16, 16, 16), C64), ((16, 16, 16), C128), ((30, 14, 22), C64)], ids=_ids)
def test_shift_bounds_and_the_other_components(hip, shape, dtype):
    rt = real_of(dtype)
    eps = np.finfo(rt).eps
    rng = np.random.RandomState(3)
    W = rng.normal(size=shape).astype(rt)
    s = orc.displacement_sets(shape, SPACING)["rms3"].astype(rt)
    plan = hip.DevicePlan(*shape, dtype)
    upload(plan, s)
    plan.upload_real(W)
    plan.particles_gather(INV_H, 1, 1.0, True)
    G = plan.particles_gather_download(1)
    c = 0.25                                                       # exactly representable
    plan.particles_shift(2, 1, c)
    Q = [plan.particles_download(a) for a in range(3)]
    add = c * G.astype(np.float64)
    assert np.all(np.abs(Q[2] - (s[2].astype(np.float64) + add)) <= 2 * eps * (np.abs(s[2]) + np.abs(add)))
    assert not np.array_equal(Q[2], s[2])
    assert np.array_equal(Q[0], s[0]) and np.array_equal(Q[1], s[1])
    assert np.array_equal(plan.particles_gather_download(1), G) and np.array_equal(plan.download_real(), W)
    # the particles have moved: a gather now answers for the new positions
    assert np.array_equal(plan.particles_gather_download(1), G)
    plan.particles_gather(INV_H, 0, 1.0, True)
    assert np.array_equal(plan.particles_gather_download(0), gorc.gather(Q, INV_H, W)[0])
    plan.close()


def test_refusals(hip):
    shape = (16, 16, 16)
    z = np.zeros(shape, np.float32)
    c2c = hip.DevicePlan(*shape, C64, unpacked=True)
    for call in (lambda: c2c.particles_gather(INV_H, 0), lambda: c2c.particles_gather_download(0), lambda: c2c.particles_shift(0, 0, 1.0),
                 lambda: c2c.set_gather_form(1)):
        with pytest.raises(RuntimeError, match="c2c"):
            call()
    data = (np.arange(16 ** 3) % 7).astype(C64).reshape(shape)
    c2c.upload_c(data)
    c2c.execute_c2c(inverse=False)
    assert np.allclose(c2c.download_c(), np.fft.fftn(data), atol=1e-2)      # still works
    c2c.close()
    ranked = hip.DevicePlan(*shape, C64, nranks=2, rank=0)
    for call in (lambda: ranked.particles_gather(INV_H, 0), lambda: ranked.particles_gather_download(0), lambda: ranked.particles_shift(0, 0, 1.0)):
        with pytest.raises(RuntimeError, match="single-rank"):
            call()
    ranked.close()
    plan = hip.DevicePlan(*shape, C64)
    lib, h = plan._lib, plan._h
    import ctypes
    dropped = ctypes.c_ulonglong(0)
    inv_h = (ctypes.c_double * 3)(*INV_H)
    assert lib.rf_particles_gather(h, None, 0, 1.0, 1, ctypes.byref(dropped)) != 0 and "null" in hip.last_error()
    assert lib.rf_particles_gather(h, inv_h, 0, 1.0, 1, None) != 0 and "null" in hip.last_error()
    assert lib.rf_particles_gather(None, inv_h, 0, 1.0, 1, ctypes.byref(dropped)) != 0 and "null" in hip.last_error()
    assert lib.rf_particles_gather_download(h, 0, None) != 0 and "null" in hip.last_error()
    assert lib.rf_particles_shift(None, 0, 0, 1.0) != 0 and "null" in hip.last_error()
    before = plan.nbytes
    plan.upload_real(z + 1)
    with pytest.raises(RuntimeError, match="no particle displacements"):
        plan.particles_gather(INV_H, 0)
    with pytest.raises(RuntimeError, match="no particle displacements"):
        plan.particles_shift(0, 0, 1.0)
    plan.close()
    plan = hip.DevicePlan(*shape, C64)
    plan.particles_upload(0, z)
    with pytest.raises(RuntimeError, match="no real-space field"):
        plan.particles_gather(INV_H, 0)
    plan.upload_real(z + 1)
    before = plan.nbytes
    for slot in (-1, 3):
        with pytest.raises(RuntimeError, match="slot"):
            plan.particles_gather(INV_H, slot)
        with pytest.raises(RuntimeError, match="slot"):
            plan.particles_gather_download(slot)
        with pytest.raises(RuntimeError, match="slot"):
            plan.particles_shift(0, slot, 1.0)
    for axis in (-1, 3):
        with pytest.raises(RuntimeError, match="axis"):
            plan.particles_shift(axis, 0, 1.0)
    for bad in ([2.0, 0.0, 2.0], [2.0, 2.0, -1.0], [np.inf, 2.0, 2.0], [2.0, np.nan, 2.0]):
        with pytest.raises(RuntimeError, match="inv_h"):
            plan.particles_gather(bad, 0)
    with pytest.raises(RuntimeError, match="form"):
        plan.set_gather_form(3)
    with pytest.raises(RuntimeError, match="no gathered values"):
        plan.particles_gather_download(0)
    with pytest.raises(RuntimeError, match="no gathered values"):
        plan.particles_shift(0, 0, 1.0)
    assert plan.nbytes == before                                   # nothing was queued or allocated
    # ... and the plan still works
    assert plan.particles_gather(INV_H, 0) == 0
    assert np.array_equal(plan.particles_gather_download(0), z + 1)
    assert plan.nbytes == before + 3 * z.nbytes
    plan.particles_shift(0, 0, 0.5)
    assert np.array_equal(plan.particles_download(0), z + 0.5)
    plan.close()


@pytest.mark.parametrize("shape", [(16, 16, 16), (40, 60, 80)], ids=_ids)
def test_generator_end_to_end(hip, shape):
    from randomfield_amd import Generator
    rt = np.float32
    eps = np.finfo(rt).eps
    gen = Generator(*shape, SPACING, rng="native", store_potential=True)
    field = gen.generate_delta_field(seed=1234, save_potential=True).copy()
    with pytest.raises(RuntimeError, match="No particle displacements"):
        gen.interpolate_at_particles()
    s = gen.particle_displacements(order=1, D1=0.5)
    last = gen.download_field().copy()                             # (the field buffer holds the last component transformed)
    got = gen.interpolate_at_particles()
    assert got.dtype == rt and got.shape == shape and gen.particles_dropped == 0
    assert np.array_equal(got, gorc.gather(s, INV_H, last)[0])
    got = gen.interpolate_at_particles(field, slot=1, coeff=COEFF)
    assert np.array_equal(got, gorc.gather(s, INV_H, field, COEFF)[0])
    got2 = gen.interpolate_at_particles(last, slot=1, coeff=-1.5, first=False)
    assert got2 is not got and np.array_equal(got2, gorc.gather(s, INV_H, last, -1.5, False, got)[0])
    assert gen.interpolate_at_particles(download=False) is None
    assert np.array_equal(gen.download_field(), last)              # the field is left as it is
    gen.shift_particles(1, coeff=0.25)                             # slot = axis
    moved = gen._download_particles()
    add = 0.25 * got2.astype(np.float64)
    assert np.all(np.abs(moved[1] - (s[1].astype(np.float64) + add)) <= 2 * eps * (np.abs(s[1]) + np.abs(add)))
    assert np.array_equal(moved[0], s[0]) and np.array_equal(moved[2], s[2])
    own = orc.displacement_sets(shape, SPACING)["rms3"].astype(rt)
    own[0][3, 4, 5] = np.nan
    gen.set_particle_displacements(own)
    got = gen.interpolate_at_particles(field, slot=2)
    want, wdrop = gorc.gather(own, INV_H, field)
    assert np.array_equal(got, want) and gen.particles_dropped == 1 == wdrop
    # a new field drops the gathered values with the displacements
    gen.generate_delta_field(seed=99, save_potential=True, download=False)
    with pytest.raises(RuntimeError, match="No particle displacements"):
        gen.interpolate_at_particles()
    gen.set_particle_displacements(own)
    with pytest.raises(RuntimeError, match="No gathered values"):
        gen.shift_particles(0)


def test_particle_mesh_force_follows_the_displacement(hip, capsys):
    """paint -> r2c -> gradient of delta_cic(k) / k^2 per axis -> gather: the particle-mesh force at the particles is the Zel'dovich
    displacement that made them, up to the CIC window (twice) and shot-noise-free non-linearity.  The numpy backend gives correlation
    coefficients 0.958 / 0.953 / 0.950 and slopes 0.85-0.88 for this field; the bound is r > 0.9 on every axis."""
    from randomfield_amd import Generator, _hip
    n, spacing, D1 = 32, 10.0, 0.1
    gen = Generator(n, n, n, spacing, rng="reference", store_potential=True)
    gen.generate_delta_field(seed=1, save_potential=True, download=False)
    s = gen.particle_displacements(order=1, D1=D1)
    painted = gen.paint_particles().copy()
    dev = gen.plan_c2r.device
    inv_h = [1.0 / spacing] * 3
    dk = 2 * np.pi / (n * spacing)
    out = []
    for axis in range(3):
        dev.upload_real(painted)
        dev.execute_r2c()
        dev.execute_gradient(axis, 1.0, dk, _hip.RF_GRAD_FROM_KSPACE)              # (forward unnormalised, inverse with 1 / N: as numpy)
        assert dev.particles_gather(inv_h, axis, 1.0, True) == 0
        force = dev.particles_gather_download(axis).astype(np.float64)
        disp = s[axis].astype(np.float64)
        r = float(np.corrcoef(force.ravel(), disp.ravel())[0, 1])
        slope = float(np.sum(force * disp) / np.sum(disp * disp))
        out.append((r, slope))
    with capsys.disabled():
        print("\nparticle-mesh loop at 32^3: (r, slope) per axis = " + ", ".join("(%.4f, %.4f)" % v for v in out))
    for r, slope in out:
        assert r > 0.9
