"""Particles on the device (rf_particles_accumulate / _upload / _download / _paint, the diagnostics rf_particles_download_counts and
rf_particles_set_paint_form; rf_k_particles.hip) and Generator.particle_displacements / paint_particles -- run with -m gpu on an MI355X.

Oracle: tests/cic_oracle.py.  The accumulator grid is integer: every form (global atomics, LDS tiles, the library's choice) must give
the oracle's grid with np.array_equal, and the field is that grid scaled and rounded once, so it is compared exactly too.  The
accumulate step: the coefficients are exactly representable, `first` is one rounding (eps/2 |coeff W|), a further add one fma rounding,
held to the two-rounding bound 2 eps (|Q| + |coeff W|) that also covers the numpy backend.

Shapes: tiled plans (16, 16, 16) both dtypes and (16, 32, 64); generic plans (4, 6, 8) both dtypes, (30, 14, 22) and (40, 60, 80):
at most 192 000 particles, one stride of every sweep.  test_generator_end_to_end also runs (64, 64, 512), 2 097 152 particles: two
strides of the global paint and of the conversion, the padded potential under calculate_displacement_field(order=1|2) and
measure_power_spectrum of the painted field on a tiled plan with nz = 512.  The forms and the accumulate step beyond one stride:
tests/test_gpu_at_scale.py."""
import numpy as np
import pytest

import cic_oracle as orc

pytestmark = pytest.mark.gpu

SPACING = 0.5            # a power of two: whole and half cells are exact in float32
INV_H = [1.0 / SPACING] * 3
C64, C128 = np.complex64, np.complex128
TILED = [((16, 16, 16), C64), ((16, 16, 16), C128), ((16, 32, 64), C64)]
GENERIC = [((4, 6, 8), C64), ((4, 6, 8), C128), ((30, 14, 22), C64), ((40, 60, 80), C64)]
FORMS = (1, 2, 0)


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


def paint_all_forms(plan, want, wdrop, rt, what):
    """A and the field under both forced forms and the library's choice: equal to each other and to the oracle"""
    field = orc.delta(want, rt)
    for form in FORMS:
        plan.set_paint_form(form)
        dropped = plan.particles_paint(INV_H)
        A = plan.particles_download_counts()
        assert dropped == wdrop, (what, form)
        assert np.array_equal(A, want), (what, form)
        assert np.array_equal(plan.download_real(), field), (what, form)
    plan.set_paint_form(0)
    return field


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_paint_every_set_every_form(hip, shape, dtype):
    rt = real_of(dtype)
    n = int(np.prod(shape))
    plan = hip.DevicePlan(*shape, dtype)
    sets = {name: s.astype(rt) for name, s in orc.displacement_sets(shape, SPACING).items()}
    for name, s in sets.items():
        want, wdrop = orc.paint(s, INV_H)
        assert wdrop == 0 and orc.total(want) == n * orc.ONE
        upload(plan, s)
        for a in range(3):
            assert np.array_equal(plan.particles_download(a), s[a])
        field = paint_all_forms(plan, want, 0, rt, name)
        if name in ("zero", "plus3", "minus2.5"):          # periodic wrap, negative wrap, half-cell split: nothing moves
            assert np.all(want == np.uint64(orc.ONE)) and not field.any()
        if name == "one":
            q = tuple(m - 1 for m in shape)
            cells = orc.one_particle(shape, q, [s[a][q] for a in range(3)], INV_H)
            hand = np.full(shape, orc.ONE, np.uint64)
            hand[q] = 0
            for cell, w in cells.items():
                hand[cell] += np.uint64(w)
            assert len(cells) == 8 and np.array_equal(want, hand)
    # one NaN and one +inf planted in the random set: dropped, counted, everything else as before
    s = sets["rms3"].copy()
    p1, p2 = (1, 2, 3), tuple(m - 1 for m in shape)
    s[1][p1] = np.nan
    s[2][p2] = np.inf
    omit = np.zeros(shape, bool)
    omit[p1] = omit[p2] = True
    want, _ = orc.paint(sets["rms3"], INV_H, omit=omit)
    assert orc.total(want) == (n - 2) * orc.ONE
    upload(plan, s)
    paint_all_forms(plan, want, 2, rt, "non-finite")
    with pytest.raises(RuntimeError, match="no realisation"):
        plan.moments()
    plan.close()


@pytest.mark.parametrize("dtype", [C64, C128], ids=_ids)
def test_every_particle_sent_to_one_point(hip, dtype):
    """maximal contention: 4096 particles' mass in the eight cells around one point, under the limit of 65536"""
    shape, rt = (16, 16, 16), real_of(dtype)
    target = np.array([5.25, 9.5, 2.75])
    s = np.empty((3,) + shape)
    for a in range(3):
        idx = np.arange(shape[a], dtype=np.float64).reshape([-1 if b == a else 1 for b in range(3)])
        s[a] = (target[a] - idx) * SPACING
    s = s.astype(rt)
    want, wdrop = orc.paint(s, INV_H)
    assert wdrop == 0 and np.count_nonzero(want) == 8 and orc.total(want) == 4096 * orc.ONE
    assert int(want[5, 9, 2]) == 4096 * (49152 * 32768 * 16384)
    plan = hip.DevicePlan(*shape, dtype)
    upload(plan, s)
    paint_all_forms(plan, want, 0, rt, "one point")
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((16, 16, 16), C64), ((16, 16, 16), C128), ((30, 14, 22), C64)], ids=_ids)
def test_accumulate_bounds_and_buffers(hip, shape, dtype):
    rt = real_of(dtype)
    eps = np.finfo(rt).eps
    n = int(np.prod(shape))
    rng = np.random.RandomState(3)
    W1, W2 = rng.normal(size=shape).astype(rt), rng.normal(size=shape).astype(rt)
    plan = hip.DevicePlan(*shape, dtype)
    plan.upload_real(W1)
    before = plan.nbytes
    with pytest.raises(RuntimeError, match="no particle displacements"):
        plan.particles_paint(INV_H)
    with pytest.raises(RuntimeError, match="no particle displacements"):
        plan.particles_download(0)
    assert plan.nbytes == before
    c1, c2 = 0.75, 0.25
    plan.particles_accumulate(1, c1, first=True)
    assert plan.nbytes == before + 3 * W1.nbytes                # Q: three arrays of the field's size
    assert np.array_equal(plan.download_real(), W1)             # W is left as it is
    Q1 = plan.particles_download(1)
    want1 = c1 * W1.astype(np.float64)
    assert np.all(np.abs(Q1 - want1) <= 0.5 * eps * np.abs(want1))
    assert not plan.particles_download(0).any() and not plan.particles_download(2).any()      # (allocated zeroed)
    plan.upload_real(W2)
    plan.particles_accumulate(1, c2, first=False)
    assert np.array_equal(plan.download_real(), W2)
    Q2 = plan.particles_download(1)
    add = c2 * W2.astype(np.float64)
    assert np.all(np.abs(Q2 - (Q1.astype(np.float64) + add)) <= 2 * eps * (np.abs(Q1) + np.abs(add)))
    plan.particles_accumulate(1, c1, first=True)                # first: what Q held does not matter
    assert np.array_equal(plan.particles_download(1), (rt(c1) * W2).astype(rt))
    plan.particles_paint(INV_H)
    assert plan.nbytes == before + 3 * W1.nbytes + 8 * n        # ... and A: 8 bytes per cell
    plan.particles_paint(INV_H)
    assert plan.nbytes == before + 3 * W1.nbytes + 8 * n
    ms = plan.kernel_ms()                                       # clear, scatter, convert
    assert len(ms) == 5 and ms[1] > 0 and ms[2] > 0 and ms[4] == 0
    with pytest.raises(RuntimeError, match="axis"):
        plan.particles_accumulate(3, 1.0, first=True)
    with pytest.raises(RuntimeError, match="form"):
        plan.set_paint_form(3)
    with pytest.raises(RuntimeError, match="inv_h"):
        plan.particles_paint([2.0, 0.0, 2.0])
    plan.close()


def test_k_buffer_and_potentials_are_untouched(hip):
    from randomfield_amd import powertools
    shape, dtype = (16, 16, 16), C64
    plan = hip.DevicePlan(*shape, dtype)
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    rng = np.random.RandomState(5)
    src = (rng.normal(size=plan.k_shape) + 1j * rng.normal(size=plan.k_shape)).astype(dtype)
    plan.upload_k(src)
    plan.save_potential()
    upload(plan, orc.displacement_sets(shape, SPACING)["small"].astype(np.float32))
    plan.particles_paint(INV_H)
    assert np.array_equal(plan.download_k(), src)
    plan.load_potential(1.0)
    pot = plan.download_k().copy()
    plan.upload_k(src)
    plan.save_potential()
    plan.load_potential(1.0)
    assert np.array_equal(plan.download_k(), pot)
    plan.close()


def test_refusals(hip):
    c2c = hip.DevicePlan(16, 16, 16, C64, unpacked=True)
    z = np.zeros((16, 16, 16), np.float32)
    with pytest.raises(RuntimeError, match="c2c"):
        c2c.particles_accumulate(0, 1.0, first=True)
    with pytest.raises(RuntimeError, match="c2c"):
        c2c.particles_upload(0, z)
    with pytest.raises(RuntimeError, match="c2c"):
        c2c.particles_download(0)
    with pytest.raises(RuntimeError, match="c2c"):
        c2c.particles_paint(INV_H)
    with pytest.raises(RuntimeError, match="c2c"):
        c2c.particles_download_counts()
    data = (np.arange(16 ** 3) % 7).astype(C64).reshape(16, 16, 16)
    c2c.upload_c(data)
    c2c.execute_c2c(inverse=False)
    assert np.allclose(c2c.download_c(), np.fft.fftn(data), atol=1e-2)      # still works
    c2c.close()
    plan = hip.DevicePlan(16, 16, 16, C64)
    with pytest.raises(RuntimeError, match="no real-space field"):
        plan.particles_accumulate(0, 1.0, first=True)
    plan.particles_upload(0, z)
    with pytest.raises(RuntimeError, match="no painted counts"):
        plan.particles_download_counts()
    plan.close()


@pytest.mark.parametrize("shape", [(16, 16, 16), (40, 60, 80), (64, 64, 512)], ids=_ids)
def test_generator_end_to_end(hip, shape):
    from randomfield_amd import Generator
    rt, D1 = np.float32, 0.5
    eps = np.finfo(rt).eps
    gen = Generator(*shape, SPACING, rng="native", store_potential=True)
    gen.generate_delta_field(seed=1234, save_potential=True, download=False)
    psi1 = [gen.calculate_displacement_field(a, order=1).astype(np.float64) for a in range(3)]
    psi2 = [gen.calculate_displacement_field(a, order=2).astype(np.float64) for a in range(3)]
    s = gen.particle_displacements(order=2, D1=D1)
    assert s.shape == (3,) + shape and s.dtype == rt
    for a in range(3):
        t1, t2 = D1 * psi1[a], D1 * D1 * psi2[a]
        assert np.all(np.abs(s[a] - (t1 + t2)) <= 2 * eps * (np.abs(t1) + np.abs(t2)))
    want, wdrop = orc.paint(s, INV_H)
    painted = gen.paint_particles().copy()
    assert gen.particles_dropped == 0 == wdrop
    assert np.array_equal(painted, orc.delta(want, rt))
    assert np.array_equal(gen.particle_positions(), orc.positions(s, SPACING))
    p_current = gen.measure_power_spectrum()
    p_given = gen.measure_power_spectrum(field=painted)
    for name in ("k", "Pk", "nmodes"):
        assert np.array_equal(p_current[name], p_given[name], equal_nan=True)
    # the state is not disturbed: the potential and the displacement calls give what they gave
    for a in range(3):
        assert np.array_equal(gen.calculate_displacement_field(a, order=1).astype(np.float64), psi1[a])
        assert np.array_equal(gen.calculate_displacement_field(a, order=2).astype(np.float64), psi2[a])
    assert gen.particle_displacements(order=1, D1=D1, download=False) is None
    first = np.stack([gen.plan_c2r.device.particles_download(a) for a in range(3)])
    for a in range(3):
        assert np.array_equal(first[a], (rt(D1) * psi1[a].astype(rt)).astype(rt))
    own = orc.displacement_sets(shape, SPACING)["rms3"].astype(rt)
    gen.set_particle_displacements(own)
    assert np.array_equal(gen.paint_particles(), orc.delta(orc.paint(own, INV_H)[0], rt))
    assert gen.paint_particles(download=False) is None
    brick, halo = gen.plan_c2r.device.paint_geometry()
    assert len(brick) == 3 and brick[2] % 64 == 0 and halo >= 1
    assert (brick[0] + 2 * halo) * (brick[1] + 2 * halo) * (brick[2] + 2 * halo) * 8 <= 160 * 1024
    # a new field drops the displacements of the old one
    gen.generate_delta_field(seed=99, save_potential=True, download=False)
    with pytest.raises(RuntimeError, match="No particle displacements"):
        gen.paint_particles()
