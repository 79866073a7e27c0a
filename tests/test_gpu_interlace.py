"""The interlaced paint on the device (rf_particles_paint_shifted, rf_kspace_stash, rf_kspace_interlace, rf_particles_paint_interlaced;
the HALF instantiations of rf_k_particles.hip's paint operations, rf_k_misc.hip interlace_kernel) and
Generator.paint_particles(interlaced=True) -- run with -m gpu on an MI355X.

Oracle: tests/interlace_oracle.py applied to the very arrays that were uploaded.  Integer atomics for the paint, float64 steps rounded
one by one for the combine: every form must give the oracle's bits, np.array_equal.  The whole call is compared bit for bit with the
sequence of public calls it stands for, and with the float64 numpy oracle within the project's transform bounds (tests/axis_matrix.py
TOL: 1e-5 rms for complex64, 3e-13 rms for complex128 -- the combine is half the sum of two such transforms with |p| <= 1).

Shapes: those of tests/test_gpu_tsc.py -- tiled plans (16, 16, 16) both dtypes and (16, 32, 128); generic plans (4, 6, 8) both dtypes
(smaller than the tile: slots alias), (30, 14, 22) and (10, 12, 70) (partial bricks, a second brick in z).  At most 65 536 particles.

A known limit of powertools.bin_power: it reads nz off the array it is given (transform.expanded_shape), which takes a packed array only
with an ODD number of stored planes, nz/2 + 1 -- so nz = 22 and nz = 70 (12 and 36 planes) are refused there, and on the numpy backend
Generator's source='kspace' cannot measure such shapes either.  rf_measure_power(RF_POWER_FROM_KSPACE) has no such limit.  For these two
shapes test_whole_call compares it with tests/power_oracle.py alone, the independent statement of the same definition that is given
the shape; for every other shape with bin_power as well.

    kernel             launch cap (source)                                  a second stride needs
    interlace_kernel   4096 x 256 threads of 16 bytes (rf_k_misc.hip        > 2 097 152 cells of the half spectrum (complex64, 2 per
                       grid_for via launch_interlace)                       lane), > 1 048 576 (complex128, 1)
test_combine_beyond_the_launch_cap opens with a regime guard, as tests/test_gpu_at_scale.py does."""
import ctypes

import numpy as np
import pytest

import axis_matrix as am
import interlace_oracle as orc
import power_oracle as po
import tsc_oracle as torc

pytestmark = pytest.mark.gpu

SPACING = 0.5
INV_H = [1.0 / SPACING] * 3
C64, C128 = np.complex64, np.complex128
TILED = [((16, 16, 16), C64), ((16, 16, 16), C128), ((16, 32, 128), C64)]
GENERIC = [((4, 6, 8), C64), ((4, 6, 8), C128), ((30, 14, 22), C64), ((10, 12, 70), C64)]
FORMS = (1, 2, 0)
SCHEMES = {"cic": 2, "tsc": 3}
K, F = 0, 1                      # RF_POWER_FROM_KSPACE, RF_POWER_FROM_FIELD
THREADS = 4096 * 256             # lanes of one stride of interlace_kernel, 16 bytes each


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else ("c64" if v == C64 else ("c128" if v == C128 else str(v)))


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
    """the displacement sets of tests/test_gpu_tsc.py rounded to the real type (once per shape and type)"""
    key = (shape, np.dtype(rt).name)
    if key not in _SETS:
        sets = dict(torc.displacement_sets(shape, SPACING))
        sets.update(torc.extra_sets(shape, SPACING))
        bad = sets["rms0.6"].copy()
        bad[1][1, 2, 3] = np.nan
        bad[2][tuple(n - 1 for n in shape)] = np.inf
        sets["non-finite"] = bad
        _SETS[key] = {name: s.astype(rt) for name, s in sets.items()}
    return _SETS[key]


def random_spectrum(kshape, dtype, seed):
    rng = np.random.RandomState(seed)
    return (rng.normal(size=kshape) + 1j * rng.normal(size=kshape)).astype(dtype)      # no Hermitian symmetry: every cell on its own


@pytest.mark.parametrize("scheme", ["cic", "tsc"])
@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_shifted_paint_every_set_every_form(hip, shape, dtype, scheme):
    rt = real_of(dtype)
    n = int(np.prod(shape))
    assert n <= 65536
    order = SCHEMES[scheme]
    plan = hip.DevicePlan(*shape, dtype)
    for name, s in sets_of(shape, rt).items():
        want, wdrop = orc.paint(s, INV_H, order)
        assert wdrop == (2 if name == "non-finite" else 0) and orc.total(want) == (n - wdrop) * orc.ONE
        upload(plan, s)
        for form in FORMS:
            plan.set_paint_form(form)
            assert plan.particles_paint(INV_H, scheme=order, half_cell=True) == wdrop, (name, form)
            A = plan.particles_download_counts()
            assert np.array_equal(A, want), (name, form)
            assert np.array_equal(plan.download_real(), orc.delta(A, rt)), (name, form)
        plan.set_paint_form(0)
    # half_cell = 0 through the new entry point is the paint of the same scheme
    s = sets_of(shape, rt)["rms3"]
    upload(plan, s)
    dropped = ctypes.c_ulonglong(9)
    inv_h = (ctypes.c_double * 3)(*INV_H)
    assert plan._lib.rf_particles_paint_shifted(plan._h, inv_h, order, 0, ctypes.byref(dropped)) == 0 and dropped.value == 0
    A0, W0 = plan.particles_download_counts(), plan.download_real()
    assert plan.particles_paint(INV_H, scheme=order) == 0
    assert np.array_equal(plan.particles_download_counts(), A0) and np.array_equal(plan.download_real(), W0)
    assert np.array_equal(A0, orc.unshifted(s, INV_H, order)[0])
    plan.close()


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_combine_alone(hip, shape, dtype):
    plan = hip.DevicePlan(*shape, dtype)
    K1, K2, K3 = (random_spectrum(plan.k_shape, dtype, seed) for seed in (1, 2, 3))
    before = plan.nbytes
    plan.upload_k(K1)
    grown = plan.nbytes
    plan.kspace_stash()
    assert plan.nbytes - grown == grown - before == K1.nbytes        # the stash is a second K, and nothing else was allocated
    assert np.array_equal(plan.download_k(), K1)
    tabs = orc.phases(shape)
    for tables, Kin in ((None, K2), (tabs, K2), (tabs, K3), ([None, tabs[1], None], K3)):
        plan.upload_k(Kin)
        plan.kspace_interlace(tables)
        assert np.array_equal(plan.download_k(), orc.combine(K1, Kin, tables))       # (the second round still uses K1)
        assert plan.elapsed_ms() >= 0
    assert plan.nbytes - grown == K1.nbytes
    plan.close()


@pytest.mark.parametrize("scheme", ["cic", "tsc"])
@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=_ids)
def test_whole_call(hip, shape, dtype, scheme):
    from randomfield_amd import powertools
    rt = real_of(dtype)
    order = SCHEMES[scheme]
    s = sets_of(shape, rt)["non-finite"]
    tabs = powertools.interlace_phases(shape)
    # the sequence of public calls on one plan ...
    ref = hip.DevicePlan(*shape, dtype)
    upload(ref, s)
    d1 = ref.particles_paint(INV_H, scheme=order, half_cell=False)
    ref.execute_r2c()
    ref.kspace_stash()
    d2 = ref.particles_paint(INV_H, scheme=order, half_cell=True)
    ref.execute_r2c()
    ref.kspace_interlace(tabs)
    ref.execute_c2r()
    Kseq, Wseq, Aseq = ref.download_k(), ref.download_real(), ref.particles_download_counts()
    ref.close()
    # ... and the one call on another
    plan = hip.DevicePlan(*shape, dtype)
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    upload(plan, s)
    assert plan.particles_paint_interlaced(INV_H, order, tabs) == d1 == d2 == 2
    assert plan.elapsed_ms() > 0
    with pytest.raises(RuntimeError, match="per-kernel"):
        plan.kernel_ms()
    Kone, Wone = plan.download_k(), plan.download_real()
    assert np.array_equal(Kone, Kseq) and np.array_equal(Wone, Wseq)
    assert np.array_equal(plan.particles_download_counts(), Aseq) and np.array_equal(Aseq, orc.paint(s, INV_H, order)[0])
    # the float64 oracle
    Kref, Wref, dropped = orc.interlaced(s, INV_H, order, rt)
    assert dropped == 2
    am.check("interlaced K " + scheme, Kone, Kref.astype(np.complex128), dtype, shape)
    am.check("interlaced field " + scheme, Wone, Wref, dtype, shape)
    am.check_moments("interlaced " + scheme, *plan.moments(), Wone.astype(np.float64), dtype, shape)
    # afterwards: K is k-space data that the measurement reads as it stands
    edges = powertools.default_k_edges(shape, SPACING, 4)
    sums = plan.measure_power(edges, K)
    po.assert_sums(sums, po.oracle(Kone, shape, SPACING, edges)[:3], "interlaced %s %s" % (_ids(shape), scheme))
    if (shape[2] // 2) % 2 == 0:         # (a known limit of bin_power, see the module docstring)
        po.assert_sums(sums, powertools.bin_power(Kone, SPACING, edges), "interlaced %s %s, bin_power" % (_ids(shape), scheme))
    assert np.array_equal(plan.download_k(), Kone) and np.array_equal(plan.download_real(), Wone)
    # the same bits on a second call, and with the other kernel form of the paint
    plan.set_paint_form(1)
    assert plan.particles_paint_interlaced(INV_H, order, tabs) == 2
    assert np.array_equal(plan.download_k(), Kone) and np.array_equal(plan.download_real(), Wone)
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((16, 16, 16), C64), ((10, 12, 70), C64), ((4, 6, 8), C128)], ids=_ids)
def test_whole_call_touches_nothing_else(hip, shape, dtype):
    from randomfield_amd import powertools
    rt = real_of(dtype)
    plan = hip.DevicePlan(*shape, dtype)
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    s = sets_of(shape, rt)["rms3"]
    upload(plan, s)
    plan.upload_k(random_spectrum(plan.k_shape, dtype, 5))
    plan.save_potential()
    plan.load_potential(1.0)
    P0 = plan.download_k().copy()
    plan.upload_real(np.random.RandomState(6).normal(size=shape).astype(rt))
    plan.particles_gather(INV_H, 1)
    G0 = plan.particles_gather_download(1).copy()
    stash = plan.download_k().nbytes
    plan.particles_paint(INV_H)                                  # (the accumulator grid and a generic plan's transform scratch ...
    plan.execute_r2c()                                           # ... exist before the call under test)
    plan.execute_c2r()
    with_a = plan.nbytes
    assert plan.particles_paint_interlaced(INV_H, 2, orc.phases(shape)) == 0
    assert plan.nbytes - with_a == stash                        # rf_plan_nbytes grew by exactly the stash
    for a in range(3):
        assert np.array_equal(plan.particles_download(a), s[a])
    assert np.array_equal(plan.particles_gather_download(1), G0)
    plan.load_potential(1.0)
    assert np.array_equal(plan.download_k(), P0)
    plan.close()


def _fresh_result(hip, shape, dtype, s, order, tabs):
    plan = hip.DevicePlan(*shape, dtype)
    upload(plan, s)
    plan.particles_paint_interlaced(INV_H, order, tabs)
    out = plan.download_k(), plan.download_real()
    plan.close()
    return out


def test_refusals_queue_nothing(hip):
    shape, dtype, rt = (16, 16, 16), C64, np.float32
    s = sets_of(shape, rt)["rms3"]
    tabs = orc.phases(shape)
    Kfresh, Wfresh = _fresh_result(hip, shape, dtype, s, 2, tabs)
    c2c = hip.DevicePlan(*shape, C64, unpacked=True)
    for call in (lambda: c2c.particles_paint(INV_H, half_cell=True), c2c.kspace_stash, c2c.kspace_interlace, lambda: c2c.particles_paint_interlaced(INV_H)):
        with pytest.raises(RuntimeError, match="c2c"):
            call()
    c2c.close()
    ranked = hip.DevicePlan(*shape, C64, nranks=2, rank=0)
    for call in (lambda: ranked.particles_paint(INV_H, half_cell=True), ranked.kspace_stash, ranked.kspace_interlace,
                 lambda: ranked.particles_paint_interlaced(INV_H)):
        with pytest.raises(RuntimeError, match="single-rank"):
            call()
    ranked.close()
    plan = hip.DevicePlan(*shape, dtype)
    empty = plan.nbytes
    for call in (lambda: plan.particles_paint(INV_H, half_cell=True), lambda: plan.particles_paint_interlaced(INV_H, 2, tabs)):
        with pytest.raises(RuntimeError, match="no particle displacements"):
            call()
    with pytest.raises(RuntimeError, match="no k-space data"):
        plan.kspace_stash()
    with pytest.raises(RuntimeError, match="no stashed spectrum"):
        plan.kspace_interlace()
    assert plan.nbytes == empty                                   # nothing was allocated
    upload(plan, s)
    loaded = plan.nbytes
    for scheme in (1, 4):
        with pytest.raises(RuntimeError, match="scheme"):
            plan.particles_paint(INV_H, scheme=scheme, half_cell=True)
        with pytest.raises(RuntimeError, match="scheme"):
            plan.particles_paint_interlaced(INV_H, scheme, tabs)
    for half in (2, -1):
        with pytest.raises(RuntimeError, match="half_cell"):
            plan.particles_paint(INV_H, half_cell=half)
    for a in range(3):
        for bad in (np.nan, np.inf):
            broken = [t.copy() for t in tabs]
            broken[a][1] = complex(0.5, bad)
            with pytest.raises(RuntimeError, match="phase table"):
                plan.particles_paint_interlaced(INV_H, 2, broken)
    assert plan.nbytes == loaded
    with pytest.raises(RuntimeError, match="no painted counts"):
        plan.particles_download_counts()
    # a stash without k-space data behind it, a combine without a stash, a combine with a bad table: K stays what it was
    src = random_spectrum(plan.k_shape, dtype, 7)
    plan.upload_k(src)
    with pytest.raises(RuntimeError, match="no stashed spectrum"):
        plan.kspace_interlace(tabs)
    plan.kspace_stash()
    broken = [t.copy() for t in tabs]
    broken[2][3] = complex(np.nan, 0.0)
    with pytest.raises(RuntimeError, match="phase table"):
        plan.kspace_interlace(broken)
    assert np.array_equal(plan.download_k(), src)
    with pytest.raises(ValueError, match="entries"):
        plan.kspace_interlace([tabs[0][:-1], None, None])
    # a combine with a stash but WITHOUT k-space data.  The gradient from k space consumes K (a tiled plan overwrote it): nothing there.
    from randomfield_amd import powertools
    other = random_spectrum(plan.k_shape, dtype, 8)
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    plan.execute_gradient(0, 1.0, 2.0 * np.pi / (shape[0] * SPACING), hip.RF_GRAD_FROM_KSPACE)
    W0 = plan.download_real()
    for call in (lambda: plan.kspace_interlace(tabs), plan.kspace_interlace, plan.download_k):
        with pytest.raises(RuntimeError, match="no k-space data"):
            call()
    assert np.array_equal(plan.download_real(), W0)
    plan.upload_k(other)
    plan.kspace_interlace(tabs)
    assert np.array_equal(plan.download_k(), orc.combine(src, other, tabs))         # the stash is what it was
    # ... and with an auxiliary REAL field in K's memory (the lensing potential): refused, that field and the stash stay what they were
    plan.execute_c2r()
    plan.lensing_potential(1.0 / (1.0 + np.arange(shape[2])), SPACING, 1)
    aux = plan.download_aux()
    with pytest.raises(RuntimeError, match="no k-space data"):
        plan.kspace_interlace(tabs)
    assert np.array_equal(plan.download_aux(), aux)
    plan.upload_k(other)
    plan.kspace_interlace(None)
    assert np.array_equal(plan.download_k(), orc.combine(src, other, None))
    lib, h = plan._lib, plan._h
    dropped = ctypes.c_ulonglong(0)
    inv_h = (ctypes.c_double * 3)(*INV_H)
    assert lib.rf_particles_paint_shifted(h, None, 2, 1, ctypes.byref(dropped)) != 0 and "null" in hip.last_error()
    assert lib.rf_particles_paint_interlaced(h, inv_h, 2, None, None, None, None) != 0 and "null" in hip.last_error()
    assert lib.rf_kspace_stash(None) != 0 and lib.rf_kspace_interlace(None, None, None, None) != 0
    # ... and the plan gives the bits of a fresh one
    assert plan.particles_paint_interlaced(INV_H, 2, tabs) == 0
    assert np.array_equal(plan.download_k(), Kfresh) and np.array_equal(plan.download_real(), Wfresh)
    plan.close()


@pytest.mark.parametrize("shape,dtype,strides", [((128, 128, 256), C64, 1), ((128, 256, 256), C64, 2), ((128, 128, 128), C128, 1)], ids=_ids)
def test_combine_beyond_the_launch_cap(hip, shape, dtype, strides):
    """the grid-stride loop of interlace_kernel and the stride's own (ix, iy, iz) with its two carries, at the smallest shapes that
    exceed the cap: by a partial second stride (both dtypes), and by a full second stride with a partial third.  Random spectra
    alone, no paint at this size."""
    vectors = shape[0] * shape[1] * (shape[2] // 2 + 1) // (2 if dtype == C64 else 1)
    assert strides * THREADS < vectors < (strides + 1) * THREADS
    plan = hip.DevicePlan(*shape, dtype)
    K1, K2 = random_spectrum(plan.k_shape, dtype, 1), random_spectrum(plan.k_shape, dtype, 2)
    tabs = orc.phases(shape)
    plan.upload_k(K1)
    plan.kspace_stash()
    plan.upload_k(K2)
    plan.kspace_interlace(tabs)
    got = plan.download_k()
    plan.close()
    assert np.array_equal(got, orc.combine(K1, K2, tabs))


@pytest.mark.parametrize("dtype", [C64, C128], ids=_ids)
@pytest.mark.parametrize("scheme", ["cic", "tsc"])
def test_generator_hip_against_numpy(hip, scheme, dtype):
    from randomfield_amd import Generator, powertools
    shape, rt = (16, 16, 16), real_of(dtype)
    s = sets_of(shape, rt)["rms0.6"]
    edges = powertools.default_k_edges(shape, SPACING, 6)
    out = {}
    for backend in ("hip", "numpy"):
        gen = Generator(*shape, SPACING, backend=backend, dtype=dtype)
        gen.set_particle_displacements(s)
        with pytest.raises(RuntimeError, match="interlaced"):
            gen.measure_power_multipoles(source="kspace")
        field = gen.paint_particles(interlaced=True, assignment=scheme).copy()
        assert gen.particles_dropped == 0
        res = gen.measure_power_multipoles(source="kspace", window=scheme, los=1, k_edges=edges)
        mono = gen.measure_power_spectrum(source="kspace", window=scheme, k_edges=edges)
        assert np.array_equal(mono["Pk"], res["P0"])
        assert np.array_equal(gen.download_field() if backend == "hip" else gen.plan_c2r.data_out, field)      # the measurement changed nothing
        with pytest.raises(ValueError, match="field"):
            gen.measure_power_spectrum(field, source="kspace")
        out[backend] = (field, res)
        if backend == "hip":
            gen.paint_particles(assignment=scheme)                # a plain paint: the spectrum is gone
            with pytest.raises(RuntimeError, match="interlaced"):
                gen.measure_power_spectrum(source="kspace")
            gen.paint_particles(interlaced=True, assignment=scheme)
        gen.measure_power_spectrum(k_edges=edges)                 # a measurement of the field: gone too, on both backends alike
        with pytest.raises(RuntimeError, match="interlaced"):
            gen.measure_power_spectrum(source="kspace")
    am.check("Generator interlaced field " + scheme, out["hip"][0], out["numpy"][0].astype(np.float64), dtype, shape)
    got, want = out["hip"][1], out["numpy"][1]
    assert np.array_equal(got["nmodes"], want["nmodes"]) and np.all(want["nmodes"] > 0)
    worst = 0.0
    for name in ("k", "P0", "P2", "P4"):
        scale = np.abs(want["P0"]) if name != "k" else np.abs(want["k"])
        err = float(np.max(np.abs(got[name] - want[name]) / scale))
        print("Generator interlaced %s %s %s: largest bin difference relative to P0 %.3e" % (scheme, _ids(dtype), name, err))
        worst = max(worst, err)
    # tests/test_gpu_power_multipoles.py test_generator_hip_backend: rtol 1e-9 (complex128); complex64 at most 1e-3
    assert worst <= (po.RTOL if dtype == C128 else 1e-3)
