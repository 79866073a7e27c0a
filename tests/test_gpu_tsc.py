"""The triangular-shaped-cloud paint and gather on the device (rf_particles_paint_ex / rf_particles_gather_ex with RF_ASSIGN_TSC;
rf_k_particles.hip TscPaintOp / TscGatherOp under cic_global_kernel / cic_tiled_kernel) and Generator(..., assignment='tsc') -- run
with -m gpu on an MI355X.

Oracle: tests/tsc_oracle.py applied to the very arrays that were uploaded.  Integer atomics for the paint, float64 steps rounded one
by one for the gather: every form -- global, LDS tiles, the library's choice -- must give the oracle's bits, np.array_equal.

Shapes: tiled plans (16, 16, 16) both dtypes and (16, 32, 128) (bricks and overlapping halos on all three axes); generic plans
(4, 6, 8) both dtypes (smaller than the tile: slots alias), (30, 14, 22) and (10, 12, 70) (partial bricks on every axis, a second
brick in z).  At most 65 536 particles."""
import ctypes

import numpy as np
import pytest

import cic_oracle as corc
import tsc_oracle as orc

pytestmark = pytest.mark.gpu

SPACING = 0.5            # a power of two: whole and half cells are exact in float32
INV_H = [1.0 / SPACING] * 3
C64, C128 = np.complex64, np.complex128
TILED = [((16, 16, 16), C64), ((16, 16, 16), C128), ((16, 32, 128), C64)]
GENERIC = [((4, 6, 8), C64), ((4, 6, 8), C128), ((30, 14, 22), C64), ((10, 12, 70), C64)]
FORMS = (1, 2, 0)
COEFF = 0.3              # not a power of two: the coefficient stays float64 inside the gather
TSC = 3


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


_SETS = {}


def sets_of(shape, rt):
    """the displacement sets rounded to the real type, one NaN and one +inf planted in a copy of the rms 0.6 set; with a field, a
    field of small integers and the oracle's paint and gathers of every set (computed once per shape and type)"""
    key = (shape, np.dtype(rt).name)
    if key not in _SETS:
        rng = np.random.RandomState(sum(shape))
        W = rng.normal(size=shape).astype(rt)
        Wint = rng.randint(-15, 16, size=shape).astype(rt)
        sets = dict(orc.displacement_sets(shape, SPACING))
        sets.update(orc.extra_sets(shape, SPACING))
        bad = sets["rms0.6"].copy()
        bad[1][1, 2, 3] = np.nan
        bad[2][tuple(n - 1 for n in shape)] = np.inf
        sets["non-finite"] = bad
        out = {}
        for name, s in sets.items():
            s = s.astype(rt)
            want, wdrop = orc.gather(s, INV_H, W)
            out[name] = (s, orc.paint(s, INV_H), (want, wdrop), orc.gather(s, INV_H, W, COEFF, False, want)[0])
        _SETS[key] = (W, Wint, out)
    return _SETS[key]


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_paint_every_set_every_form(hip, shape, dtype):
    rt = real_of(dtype)
    n = int(np.prod(shape))
    assert n <= 65536
    _, _, sets = sets_of(shape, rt)
    plan = hip.DevicePlan(*shape, dtype)
    for name, (s, (want, wdrop), _, _) in sets.items():
        assert wdrop == (2 if name == "non-finite" else 0)
        upload(plan, s)
        for form in FORMS:
            plan.set_paint_form(form)
            assert plan.particles_paint(INV_H, scheme=TSC) == wdrop, (name, form)
            A = plan.particles_download_counts()
            assert np.array_equal(A, want), (name, form)
            assert np.array_equal(plan.download_real(), orc.delta(A, rt)), (name, form)
            assert orc.total(A) == (n - wdrop) * orc.ONE, (name, form)
        plan.set_paint_form(0)
        if name in ("zero", "plus3", "minus2.5"):
            assert np.all(want == np.uint64(orc.ONE)), name
    # a cloud-in-cell paint directly after a TSC paint on the same plan
    s = sets["rms3"][0]
    upload(plan, s)
    plan.particles_paint(INV_H, scheme=TSC)
    assert plan.particles_paint(INV_H) == 0
    assert np.array_equal(plan.particles_download_counts(), corc.paint(s, INV_H)[0])
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((16, 16, 16), C64), ((10, 12, 70), C64), ((4, 6, 8), C128)], ids=_ids)
def test_single_displaced_particle_by_hand(hip, shape, dtype):
    """the last cell's particle displaced by (0.3, 1.75, -0.6) cells, every other particle left out through a NaN: its 27 cells with
    the weights of the definition worked out here in Python integers"""
    rt = real_of(dtype)
    q = tuple(n - 1 for n in shape)
    s = np.full((3,) + shape, np.nan, rt)
    disp = (np.array([0.3, 1.75, -0.6]) * SPACING).astype(rt)
    s[(slice(None),) + q] = disp
    per_axis = []
    for a in range(3):
        u = float(disp[a]) * INV_H[a]
        c = int(np.floor(u))
        t = int(np.floor((u - c) * 65536.0))
        up = t >= 32768
        tau = t - 32768 if up else t + 32768
        jc = (q[a] + c + (1 if up else 0)) % shape[a]
        wm, wp = ((65536 - tau) ** 2) >> 17, (tau ** 2) >> 17
        per_axis.append([((jc - 1) % shape[a], wm), (jc, 65536 - wm - wp), ((jc + 1) % shape[a], wp)])
    # u = 0.3: the own cell is the centre; 1.75: the centre is two cells up; -0.6: one cell down
    assert [p[1][0] for p in per_axis] == [q[0], (q[1] + 2) % shape[1], (q[2] - 1) % shape[2]]
    want = np.zeros(shape, np.uint64)
    for jx, wx in per_axis[0]:
        for jy, wy in per_axis[1]:
            for jz, wz in per_axis[2]:
                want[jx, jy, jz] += np.uint64(wx * wy * wz)
    assert orc.total(want) == orc.ONE and np.count_nonzero(want) == 27
    plan = hip.DevicePlan(*shape, dtype)
    upload(plan, s)
    for form in FORMS:
        plan.set_paint_form(form)
        assert plan.particles_paint(INV_H, scheme=TSC) == s[0].size - 1
        assert np.array_equal(plan.particles_download_counts(), want), form
    plan.close()


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_gather_every_set_every_form(hip, shape, dtype):
    rt = real_of(dtype)
    W, Wint, sets = sets_of(shape, rt)
    plan = hip.DevicePlan(*shape, dtype)
    for name, (s, (A, _), (want, wdrop), want_add) in sets.items():
        upload(plan, s)
        plan.upload_real(W)
        for form in FORMS:
            plan.set_gather_form(form)
            slot = form                                                # (every slot is used)
            assert plan.particles_gather(INV_H, slot, 1.0, True, scheme=TSC) == wdrop, (name, form)
            assert np.array_equal(plan.particles_gather_download(slot), want), (name, form)
            assert plan.particles_gather(INV_H, slot, COEFF, False, scheme=TSC) == wdrop, (name, form)
            assert np.array_equal(plan.particles_gather_download(slot), want_add), (name, form)
        plan.set_gather_form(0)
        # the adjoint identity against the TSC paint of the same Q: sum_q g 2^48 == sum_cells A W in integers (|W| <= 15: every
        # step exact; checked on the device's own G for float64 plans and through the oracle's exact g for float32, as for cloud in cell)
        plan.upload_real(Wint)
        plan.particles_gather(INV_H, 0, 1.0, True, scheme=TSC)
        G = plan.particles_gather_download(0)
        g, keep = orc.gather_g(s, INV_H, Wint)
        g = np.where(keep, g, 0.0)
        assert np.array_equal(G, g.astype(rt)), name
        rhs = sum(int(a) * int(w) for a, w in zip(A.ravel(), Wint.ravel()))
        scaled = (G.astype(np.float64) if rt == np.float64 else g) * 2.0 ** 48
        assert np.all(scaled == np.floor(scaled)) and sum(int(v) for v in scaled.ravel()) == rhs, name
    # a constant field of 3 gathers exactly 3
    upload(plan, sets["rms3"][0])
    plan.upload_real(np.full(shape, 3, rt))
    for form in FORMS:
        plan.set_gather_form(form)
        plan.particles_gather(INV_H, 1, 1.0, True, scheme=TSC)
        assert np.all(plan.particles_gather_download(1) == 3), form
    # a NaN in W reaches every particle whose 27 cells contain it, also through a zero weight: every particle (-0.5 + 100 / 65536)
    # cells off its lattice point has tau = 100 and Wp = 0, and the particle one cell below the NaN sees it through that weight alone
    p = (1, 2, 3)
    Wn = W.copy()
    Wn[p] = np.nan
    s = np.full((3,) + shape, (-0.5 + 100 / 65536.0) * SPACING).astype(rt)
    want, _ = orc.gather(s, INV_H, Wn)
    assert np.isnan(want[0, 1, 2]) and np.count_nonzero(np.isnan(want)) == 27
    upload(plan, s)
    plan.upload_real(Wn)
    for form in FORMS:
        plan.set_gather_form(form)
        plan.particles_gather(INV_H, 2, 1.0, True, scheme=TSC)
        assert np.array_equal(plan.particles_gather_download(2), want, equal_nan=True), form
    plan.close()


def test_gather_changes_nothing_but_the_slot(hip):
    from randomfield_amd import powertools
    shape, dtype, rt = (16, 16, 16), C64, np.float32
    plan = hip.DevicePlan(*shape, dtype)
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    rng = np.random.RandomState(5)
    src = (rng.normal(size=plan.k_shape) + 1j * rng.normal(size=plan.k_shape)).astype(dtype)
    plan.upload_k(src)
    s = sets_of(shape, rt)[2]["rms3"][0]
    upload(plan, s)
    plan.particles_paint(INV_H, scheme=TSC)

    def state():
        return [plan.download_real().copy()] + [plan.particles_download(a).copy() for a in range(3)] + [plan.particles_download_counts().copy(),
                                                                                                       plan.download_k().copy()]

    was = state()
    assert np.array_equal(was[4], orc.paint(s, INV_H)[0])
    for form in FORMS:
        plan.set_gather_form(form)
        plan.particles_gather(INV_H, 2, 1.0, True, scheme=TSC)
        plan.particles_gather(INV_H, 2, COEFF, False, scheme=TSC)
        for a, b in zip(was, state()):
            assert np.array_equal(a, b), form
    assert np.array_equal(plan.particles_gather_download(2), orc.gather(s, INV_H, was[0], COEFF, False, orc.gather(s, INV_H, was[0])[0])[0])
    ms = plan.kernel_ms()                                          # the gather alone, as for cloud in cell
    assert len(ms) == 5 and ms[0] > 0 and ms[4] == 0
    plan.close()


def test_refused_schemes_queue_nothing(hip):
    shape, rt = (16, 16, 16), np.float32
    plan = hip.DevicePlan(*shape, C64)
    W, _, sets = sets_of(shape, rt)
    s = sets["rms3"][0]
    upload(plan, s)
    plan.upload_real(W)
    before = plan.nbytes
    for scheme in (1, 4):
        with pytest.raises(RuntimeError, match="scheme"):
            plan.particles_paint(INV_H, scheme=scheme)
        with pytest.raises(RuntimeError, match="scheme"):
            plan.particles_gather(INV_H, 0, scheme=scheme)
    assert plan.nbytes == before                                   # neither the accumulator grid nor G was allocated
    with pytest.raises(RuntimeError, match="no painted counts"):
        plan.particles_download_counts()
    with pytest.raises(RuntimeError, match="no gathered values"):
        plan.particles_gather_download(0)
    assert np.array_equal(plan.download_real(), W)
    lib, h = plan._lib, plan._h
    dropped = ctypes.c_ulonglong(0)
    inv_h = (ctypes.c_double * 3)(*INV_H)
    assert lib.rf_particles_paint_ex(h, None, TSC, ctypes.byref(dropped)) != 0 and "null" in hip.last_error()
    assert lib.rf_particles_gather_ex(h, inv_h, TSC, 0, 1.0, 1, None) != 0 and "null" in hip.last_error()
    assert lib.rf_particles_gather_ex(h, inv_h, TSC, 3, 1.0, 1, ctypes.byref(dropped)) != 0 and "slot" in hip.last_error()
    # ... and the plan still works, with the scheme constants of the header
    assert lib.rf_particles_gather_ex(h, inv_h, 2, 0, 1.0, 1, ctypes.byref(dropped)) == 0
    import gather_oracle as gorc
    assert np.array_equal(plan.particles_gather_download(0), gorc.gather(s, INV_H, W)[0])
    assert plan.particles_gather(INV_H, 0, scheme=TSC) == 0
    assert np.array_equal(plan.particles_gather_download(0), sets["rms3"][2][0])
    plan.close()


def test_generator_paints_measures_and_interpolates(hip):
    from randomfield_amd import Generator
    shape, rt = (16, 16, 16), np.float32
    s = sets_of(shape, rt)[2]["non-finite"][0]
    A, wdrop = orc.paint(s, INV_H)
    fields = {}
    for backend in ("hip", "numpy"):
        gen = Generator(*shape, SPACING, backend=backend) if backend == "numpy" else Generator(*shape, SPACING, rng="native")
        field = gen.generate_delta_field(seed=3, save_potential=True).copy()
        gen.set_particle_displacements(s)
        painted = gen.paint_particles(assignment="tsc").copy()
        assert np.array_equal(painted, orc.delta(A, rt)) and gen.particles_dropped == wdrop == 2, backend
        if backend == "hip":
            assert np.array_equal(gen.plan_c2r.device.particles_download_counts(), A)
        res = gen.measure_power_spectrum(window="tsc")
        assert len(res) and np.all(np.isfinite(res["Pk"][res["nmodes"] > 0])), backend
        fields[backend] = res
        got = gen.interpolate_at_particles(painted, slot=1, coeff=COEFF, assignment="tsc")
        assert np.array_equal(got, orc.gather(s, INV_H, painted, COEFF)[0]), backend
        with pytest.raises(ValueError, match="assignment"):
            gen.paint_particles(assignment="pcs")
    assert np.array_equal(fields["hip"]["nmodes"], fields["numpy"]["nmodes"])      # (the same modes; both measured delta(A) of one A)
