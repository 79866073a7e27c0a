"""Generic grids with the generation inside the first FFT pass (RF_FLAG_FUSED_GENERIC_GENERATION; rf_generic.h generic_c2r_from_seq,
rf_k_generic.hip generic_axis_gen_kernel) -- run with -m gpu on an MI355X.

The fused realisation must be the unfused one bit for bit: the same gen_cell values go to the same LDS positions and through the same
stages and stores; only where the x pass takes them from differs.  The shapes are the smallest that reach each launch class of the
x pass (rf_k_generic.hip strided_shape; tests/test_gpu_generic.py lists the classes): tile 16 / 8 / 4 lines per workgroup, in place
and two-buffer lines, a ragged last workgroup, fewer lines than a tile, and an x axis in the four-step form, which is not fused.
"""
import numpy as np
import pytest

from conftest import golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-5          # * rms: the tolerances of tests/test_gpu_generic.py
TOL_F64 = 1e-11
SPACING = 0.5

C64, C128 = np.complex64, np.complex128
EQUAL = [((4, 6, 8), C64), ((4, 6, 8), C128),                 # one workgroup, 20 lines of 4 points
         ((40, 60, 80), C64), ((40, 60, 80), C128),           # the reference's own test shape: tile 16, in place
         ((30, 14, 22), C64),                                 # 168 lines: a ragged last workgroup at tile 16
         ((154, 28, 44), C64), ((154, 28, 44), C128),         # 2 7 11: not smooth, two LDS buffers
         ((1200, 30, 40), C64),                               # tile 8, 1024 threads, LDS beyond 64 KB
         ((1200, 6, 8), C128), ((2400, 6, 8), C64),           # tile 4: 30 lines, fewer than 16 per workgroup
         ((2000, 6, 8), C128), ((4000, 10, 24), C64),         # two lines per workgroup: four-step by preference -- x is split, the fallback runs
         ((16384, 4, 6), C64)]                                # x beyond one LDS line: split, the flag accepted and harmless


def _tag(dtype):
    return "c64" if dtype == C64 else "c128"


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else _tag(v)


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def dpower():
    d = golden("default_power.npz")
    return d["k"], d["Pk"]


def make_plan(hip, shape, dtype, k, Pk, spacing=SPACING):
    from randomfield_amd import powertools
    nx, ny, nz = shape
    plan = hip.DevicePlan(nx, ny, nz, dtype)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, spacing))
    xt, st = cpu_ref.sigma_table(k, Pk, nx, ny, nz, spacing)
    plan.set_power(xt, st)
    return plan


def _realise(plan, seed, noise):
    if noise is None:
        plan.realise(seed=seed)
    else:
        plan.realise(noise=noise)
    return plan.download_real(), plan.moments()


@pytest.mark.parametrize("shape,dtype", EQUAL, ids=_ids)
def test_fused_equals_unfused_bit_for_bit(hip, dpower, shape, dtype):
    nx, ny, nz = shape
    k, Pk = dpower
    seed = 31337
    noise = cpu_ref.reference_noise(11, nx * ny * (nz // 2 + 1))
    plan = make_plan(hip, shape, dtype, k, Pk)
    try:
        assert not plan.tiled and plan.fused_generation is False
        for exact in (False, True):
            plan.set_exact_generation(exact)
            for nz_ in (None, noise):                              # native seed; resident float64 deviates
                plan.set_fused_generation(False)
                want, wm = _realise(plan, seed, nz_)
                plan.set_fused_generation(True)
                assert plan.fused_generation is True
                got, gm = _realise(plan, seed, nz_)
                assert float(np.std(want)) > 0
                assert np.array_equal(got, want), "exact=%s noise=%s" % (exact, nz_ is not None)
                assert gm == wm
        plan.set_exact_generation(False)
        plan.set_fused_generation(False)
        want, wm = _realise(plan, seed, None)
        plan.set_fused_generation(True)
        rms_b = plan.realise_batch([1, 2, seed])                   # the generic branch of rf_realise_batch
        assert rms_b[2] == wm[1] and np.array_equal(plan.download_real(), want)
        assert rms_b[0] != rms_b[1] and rms_b[1] != rms_b[2]
    finally:
        plan.close()


@pytest.mark.parametrize("dtype", [C64, C128], ids=_tag)
def test_fused_field_against_oracle(hip, dpower, dtype):
    shape = (100, 150, 200)
    nx, ny, nz = shape
    k, Pk = dpower
    seed = 31337
    tol = TOL_F32 if dtype == C64 else TOL_F64
    noise = cpu_ref.native_noise(seed, nx, ny, nz, dtype)
    ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=dtype, double_fft=True)
    del noise
    rms = float(rms)
    plan = make_plan(hip, shape, dtype, k, Pk)
    try:
        plan.set_fused_generation(True)
        plan.realise(seed=seed)
        err = float(np.max(np.abs(plan.download_real() - ref))) / rms
        std = plan.moments()[1]
        print("%s %s fused native fast err %.3g * rms, |std - rms| %.3g * rms" % (shape, _tag(dtype), err, abs(std - rms) / rms))
        assert err <= 1e-5
        assert abs(std - rms) <= 1e-5 * rms
        plan.set_exact_generation(True)
        plan.realise(seed=seed)
        xerr = float(np.max(np.abs(plan.download_real() - ref))) / rms
        print("%s %s fused native exact err %.3g * rms" % (shape, _tag(dtype), xerr))
        assert xerr <= tol
        assert abs(plan.moments()[1] - rms) <= tol * rms
    finally:
        plan.close()


def test_fused_realisation_leaves_no_k_space(hip, dpower):
    k, Pk = dpower
    plan = make_plan(hip, (40, 60, 80), C64, k, Pk)
    try:
        plan.set_fused_generation(True)
        plan.realise(seed=5)
        with pytest.raises(RuntimeError, match="no k-space data"):
            plan.download_k()
        plan.realise_batch([5, 6])
        with pytest.raises(RuntimeError, match="no k-space data"):
            plan.download_k()
        plan.generate(seed=5)                                      # unaffected by the flag: the array is there again
        ks = plan.download_k()
        assert cpu_ref.is_hermitian_packed(ks, rtol=0, atol=0) and float(np.abs(ks).max()) > 0
        plan.realise(seed=6)                                       # ... and a fused realisation leaves it as it was
        assert np.array_equal(plan.download_k(), ks)
    finally:
        plan.close()


def test_flag_is_refused_where_it_does_not_apply(hip):
    tiled = hip.DevicePlan(16, 16, 16, C64)
    try:
        assert tiled.tiled
        with pytest.raises(RuntimeError, match="generic"):
            tiled.set_fused_generation(True)
        assert tiled.fused_generation is False
    finally:
        tiled.close()
    c2c = hip.DevicePlan(6, 10, 12, C64, unpacked=True)
    try:
        with pytest.raises(RuntimeError, match="generic"):
            c2c.set_fused_generation(True)
        assert c2c.fused_generation is False
    finally:
        c2c.close()


def test_kernel_ms_on_a_generic_plan(hip, dpower):
    k, Pk = dpower
    plan = make_plan(hip, (40, 60, 80), C64, k, Pk)
    try:
        plan.realise(seed=5)
        ms = plan.kernel_ms()
        print("unfused kernel_ms", ms)
        assert len(ms) == 5 and all(ms[i] > 0 for i in (0, 1, 2)) and ms[4] > 0
        plan.set_fused_generation(True)
        plan.realise(seed=5)
        ms = plan.kernel_ms()
        print("fused kernel_ms", ms)
        assert all(ms[i] > 0 for i in (0, 1, 2)) and ms[4] == 0.0
    finally:
        plan.close()


@pytest.mark.parametrize("rng", ["native", "reference"])
def test_generator_fields_do_not_depend_on_the_option(hip, rng):
    from randomfield_amd import Generator
    nz = 80                                                        # (generate_density_field needs the two O(nz) background tables)
    gen = Generator(40, 60, nz, 2.5, rng=rng, growth_function=np.linspace(1.0, 0.6, nz), mean_matter_density=np.linspace(1.0, 2.0, nz))
    dev = gen.plan_c2r.device
    assert not dev.tiled
    out = {}
    for on in (False, True):
        dev.set_fused_generation(on)
        delta = np.array(gen.generate_delta_field(seed=123, save_potential=False))
        out[on] = (delta, gen.delta_field_rms, np.array(gen.generate_density_field(seed=123)))
    assert float(np.std(out[False][0])) > 0
    assert np.array_equal(out[True][0], out[False][0])
    assert out[True][1] == out[False][1]
    assert np.array_equal(out[True][2], out[False][2])
