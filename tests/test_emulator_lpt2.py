"""The second-order (2LPT) displacement on the CPU: the Hessian cell function over an array from both sources (emu_hessian_k, rf_core.h
hess_cell), the generic sequence that applies it inside the x pass (rf_generic.h generic_c2r_from_seq, GenericDerivSource) against
"elementwise, then generic_c2r_seq" bit for bit, the accumulate step function (emu_lpt2_accumulate, rf_core.h lpt2_step), the numpy
backend of Generator.lpt2_source / calculate_displacement_field(order=2) against tests/lpt2_oracle.py, and the ABI surface (feature
bit 16, version still 5.5).  No GPU needed.

Tolerances.  Elementwise: two roundings (the factor, the product), 4 eps as the gradient's.  Accumulate: the chain s = t h ... has at
most 11 roundings of at most eps/2 of A(x) = sum |the six products| each; 8 eps A(x) is the margin.  Fields: TOL = 1e-5 (float32) /
1e-11 (float64) times the rms per transform, the generic path's own (tests/test_gpu_generic.py).  The source S is a sum of products
of two transformed fields, so its bound is per cell: TOL * sum_{a<b} (|H_aa| rms_bb + |H_bb| rms_aa + 2 |H_ab| rms_ab) + 8 eps A(x),
from the oracle's own components.  psi2 against the oracle applied to the code's own S: 2 TOL rms (two transforms)."""
import ctypes

import numpy as np
import pytest

import emu_util
import lpt2_oracle as orc
from randomfield_amd import transform

SPACING = 2.5
C64, C128 = np.complex64, np.complex128
K_SHAPES = [(4, 6, 8), (6, 4, 12), (16, 16, 16)]
SEQ_SHAPES = [(4, 6, 8), (40, 60, 80), (30, 14, 22)]
TOL = {C64: 1e-5, C128: 1e-11}
FIRST, DIAG2, DIAG3, OFF, LAST = range(5)
STEPS = [FIRST, DIAG2, DIAG3, OFF, OFF, LAST]

_c_dp = ctypes.POINTER(ctypes.c_double)
_HEAD = [ctypes.c_int] * 6 + [ctypes.c_double] * 3 + [ctypes.c_int, _c_dp, _c_dp, _c_dp, ctypes.c_void_p, ctypes.c_longlong]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else ("c64" if v == C64 else "c128")


def real_of(dtype):
    return np.float32 if dtype == C64 else np.float64


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_hessian_k.argtypes = _HEAD + [ctypes.c_void_p]
    lib.emu_hessian_k.restype = ctypes.c_int
    lib.emu_generic_hessian_c2r.argtypes = _HEAD + [ctypes.c_void_p, _c_dp, _c_dp]
    lib.emu_generic_hessian_c2r.restype = ctypes.c_int
    lib.emu_lpt2_accumulate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    lib.emu_lpt2_accumulate.restype = ctypes.c_int
    return lib


def spectrum(shape, dtype, seed=3):
    """a random Hermitian half spectrum (as tests/test_emulator_gradient.py)"""
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


def potential_of(src, shape):
    k2 = orc.ksq_grid(shape, SPACING)
    k2[0, 0, 0] = 1.0
    pot = (src / k2).astype(src.dtype)
    pot[0, 0, 0] = 0
    return pot


def _args(shape, dtype, a, b, scale, divide, src, pitch=None):
    from randomfield_amd import powertools
    nx, ny, nz = shape
    kx2, ky2, kz2 = (np.ascontiguousarray(t, np.float64) for t in powertools.ksq_axes(*shape, SPACING))
    dk = orc.dk_of(shape, SPACING)
    pitch = nz // 2 + 1 if pitch is None else pitch
    return (int(dtype == C128), nx, ny, nz, a, b, float(scale), dk[a], dk[b], int(divide), emu_util._dp(kx2), emu_util._dp(ky2),
            emu_util._dp(kz2), src.ctypes.data_as(ctypes.c_void_p), pitch), (kx2, ky2, kz2, src)


def hessian_k(lib, src, shape, a, b, scale, divide, pitch=None):
    args, keep = _args(shape, src.dtype.type, a, b, scale, divide, src, pitch)
    out = np.empty((shape[0], shape[1], shape[2] // 2 + 1), src.dtype)
    assert lib.emu_hessian_k(*args, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def hessian_field(lib, src, shape, a, b, scale, divide, pitch=None):
    args, keep = _args(shape, src.dtype.type, a, b, scale, divide, src, pitch)
    out = np.empty(shape, real_of(src.dtype))
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    assert lib.emu_generic_hessian_c2r(*args, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(s1), ctypes.byref(s2)) == 0
    return out, s1.value, s2.value


def assert_elementwise(got, want, factor, dtype):
    eps = np.finfo(real_of(dtype)).eps
    zero = np.broadcast_to(factor == 0, got.shape)
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        err = np.abs(g.astype(np.float64) - w)
        nzw = w != 0
        print("elementwise: max err / (eps |want|) = %.3f" % np.max(err[nzw] / (eps * np.abs(w[nzw]))))
        assert np.all(err <= 4 * eps * np.abs(w))
        assert np.all(g[zero] == 0)


@pytest.mark.parametrize("dtype", [C64, C128], ids=_ids)
@pytest.mark.parametrize("shape", K_SHAPES, ids=_ids)
def test_hessian_k_elementwise_all_pairs_both_sources(lib, shape, dtype):
    src = spectrum(shape, dtype)
    scale = -1.75
    for a, b in orc.PAIRS:
        factor = orc.hessian_factor(shape, SPACING, a, b, scale)
        assert np.any(factor == 0) and factor[0, 0, 0] == 0
        for divide in (0, 1):
            got = hessian_k(lib, src, shape, a, b, scale, divide)
            assert_elementwise(got, orc.hessian_k(src, shape, SPACING, a, b, scale, bool(divide)), factor, dtype)
            assert transform.is_hermitian(got, packed=True)
            assert float(np.abs(got).max()) > 0
    # the diagonal drops its own Nyquist plane too
    assert np.all(hessian_k(lib, src, shape, 0, 0, 1.0, 0)[shape[0] // 2] == 0)
    with_bad_axes = _args(shape, dtype, 1, 0, 1.0, 0, src)[0]
    assert lib.emu_hessian_k(*with_bad_axes, src.ctypes.data_as(ctypes.c_void_p)) != 0


def test_hessian_k_reads_a_padded_source_and_works_in_place(lib):
    shape = (6, 4, 12)
    src = spectrum(shape, C64)
    padded = np.full((6, 4, 10), np.nan + 0j, C64)
    padded[:, :, :7] = src
    assert np.array_equal(hessian_k(lib, padded, shape, 0, 1, 2.0, 0, pitch=10), hessian_k(lib, src, shape, 0, 1, 2.0, 0))
    want = hessian_k(lib, src, shape, 1, 2, 1.0, 1)
    args, keep = _args(shape, C64, 1, 2, 1.0, 1, src)
    assert lib.emu_hessian_k(*args, src.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(src, want)


@pytest.mark.parametrize("dtype", [C64, C128], ids=_ids)
@pytest.mark.parametrize("shape", SEQ_SHAPES, ids=_ids)
def test_fused_sequence_equals_elementwise_then_c2r_bit_for_bit(lib, shape, dtype):
    src = spectrum(shape, dtype)
    pot = potential_of(src, shape)
    for a, b in orc.PAIRS:
        for divide, source in ((0, pot), (1, src)):
            oracle = orc.irfftn(orc.hessian_k(source, shape, SPACING, a, b, 1.0, bool(divide)), shape)
            rms = float(np.std(oracle))
            assert rms > 0
            for walk in (None, (16, 16)):
                if walk is None:
                    want, w1, w2 = emu_util.generic_c2r(hessian_k(lib, source, shape, a, b, 1.0, divide))
                    got, g1, g2 = hessian_field(lib, source, shape, a, b, 1.0, divide)
                else:
                    with emu_util.generic_threads(*walk):
                        want, w1, w2 = emu_util.generic_c2r(hessian_k(lib, source, shape, a, b, 1.0, divide))
                        got, g1, g2 = hessian_field(lib, source, shape, a, b, 1.0, divide)
                assert got.dtype == real_of(dtype) and np.array_equal(got, want), (a, b, divide, walk)
                assert (g1, g2) == (w1, w2)
                err = float(np.max(np.abs(got - oracle)))
                print("field: H_%d%d divide %d walk %s max err / rms = %.3g" % (a, b, divide, walk, err / rms))
                assert err <= TOL[dtype] * rms
    nzh = shape[2] // 2 + 1
    padded = np.zeros(shape[:2] + (nzh + 2,), dtype)
    padded[:, :, :nzh] = pot
    assert np.array_equal(hessian_field(lib, padded, shape, 0, 2, 1.0, 0, pitch=nzh + 2)[0], hessian_field(lib, pot, shape, 0, 2, 1.0, 0)[0])


def test_split_x_axis_takes_the_unfused_fallback(lib):
    shape = (40, 60, 80)
    pot = spectrum(shape, C64)
    old = lib.emu_set_generic_cap(16)
    try:
        want = emu_util.generic_c2r(hessian_k(lib, pot, shape, 0, 1, 1.0, 0))[0]
        got = hessian_field(lib, pot, shape, 0, 1, 1.0, 0)[0]
    finally:
        lib.emu_set_generic_cap(old)
    assert np.array_equal(got, want)
    plain = hessian_field(lib, pot, shape, 0, 1, 1.0, 0)[0]
    assert not np.array_equal(got, plain) and np.max(np.abs(got - plain)) <= 1e-5 * float(np.std(plain))


@pytest.mark.parametrize("rt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [4096, 1003], ids=["whole_blocks", "ragged"])
def test_accumulate_steps_against_float64(lib, rt, n):
    """n = 1003: not a multiple of the kernel's cells per block (256 lanes x 16 bytes), nor of a lane's"""
    rng = np.random.RandomState(7)
    comps = [(rng.normal(size=n) * 10.0 ** rng.uniform(-2, 2, size=n)).astype(rt) for _ in range(6)]
    T, S = np.full(n, np.nan, rt), np.full(n, np.nan, rt)
    for h, step in zip(comps, STEPS):
        W = h.copy()
        assert lib.emu_lpt2_accumulate(int(rt == np.float64), step, W.ctypes.data_as(ctypes.c_void_p), T.ctypes.data_as(ctypes.c_void_p),
                                       S.ctypes.data_as(ctypes.c_void_p), n) == 0
        if step != LAST:
            assert np.array_equal(W, h)                       # only the last step writes the field buffer
    H = {ab: c.astype(np.float64) for ab, c in zip(orc.PAIRS, comps)}
    want, A = orc.source_from(H), orc.source_magnitude(H)
    err = np.abs(W.astype(np.float64) - want)
    print("accumulate: max err / (eps A) = %.3f" % np.max(err / (np.finfo(rt).eps * A)))
    assert np.all(err <= 8 * np.finfo(rt).eps * A)
    assert lib.emu_lpt2_accumulate(0, 5, W.ctypes.data_as(ctypes.c_void_p), T.ctypes.data_as(ctypes.c_void_p), S.ctypes.data_as(ctypes.c_void_p), n) != 0


# ---- the oracle's own identities (float64) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 6, 8), (16, 16, 16), (30, 14, 22)], ids=_ids)
def test_oracle_identities(shape):
    phi = potential_of(spectrum(shape, C128), shape)
    S = orc.source(phi, shape, SPACING)
    rms = float(np.std(S))
    assert abs(S.mean()) <= 3e-17 * rms
    psi = [orc.displacement2(phi, shape, SPACING, a) for a in range(3)]
    k2 = orc.ksq_grid(shape, SPACING)
    k2[0, 0, 0] = 1.0
    want = -(3.0 / 7.0) * orc.irfftn(orc.rfftn(S) * orc.dropped_ksq(shape, SPACING) / k2, shape)
    assert np.max(np.abs(orc.divergence(psi, shape, SPACING) - want)) <= 3e-15 * rms
    two, closed = orc.two_wave_potential(shape, SPACING, 1.5, -0.7, 1, 1)
    assert np.max(np.abs(orc.source(two, shape, SPACING) - closed)) <= 1e-14
    if min(shape) >= 6:
        wave = orc.oblique_wave_potential(shape, SPACING, 2.0, (1, 2, 1))
        H = orc.hessian_fields(wave, shape, SPACING)
        assert np.all(np.abs(orc.source_from(H)) <= source_bound(H, C128)) and np.max(orc.source_magnitude(H)) > 0


# ---- numpy backend of the Generator ------------------------------------------------------------------------------------------
def source_bound(H, dtype):
    """per cell: what two transformed factors held to TOL * rms each, and the sweep's roundings, can move S by"""
    rms = {ab: float(np.std(h)) for ab, h in H.items()}
    lin = sum(np.abs(H[a, a]) * rms[b, b] + np.abs(H[b, b]) * rms[a, a] + 2 * np.abs(H[a, b]) * rms[a, b] for a, b in ((0, 1), (0, 2), (1, 2)))
    return TOL[dtype] * lin + 8 * np.finfo(real_of(dtype)).eps * orc.source_magnitude(H)


def numpy_generator(shape, dtype, potential=None, seed=11):
    from randomfield_amd import Generator
    gen = Generator(*shape, SPACING, backend="numpy", dtype=dtype)
    if potential is None:
        gen.generate_delta_field(seed=seed, save_potential=True)
    else:
        gen.potential = np.asarray(potential, dtype)                # an uploaded potential
    return gen


def check_generator_against_oracle(gen, shape, dtype):
    pot = np.asarray(gen.potential, C128)
    H = orc.hessian_fields(pot, shape, SPACING)
    S = gen.lpt2_source().copy()
    assert S.shape == shape and S.dtype == real_of(dtype)
    err = np.abs(S.astype(np.float64) - orc.source_from(H))
    bound = source_bound(H, dtype)
    print("source: max err / bound = %.3g" % np.max(err / bound))
    assert np.all(err <= bound)
    rms = float(np.std(S))
    assert abs(float(S.astype(np.float64).mean())) <= TOL[dtype] * rms
    for axis in range(3):
        want = orc.displacement2_from_source(S, shape, SPACING, axis)
        got = gen.calculate_displacement_field(axis, order=2).copy()
        e = float(np.max(np.abs(got - want)))
        print("psi2 axis %d: max err / rms = %.3g" % (axis, e / np.std(want)))
        assert e <= 2 * TOL[dtype] * float(np.std(want))
    return S


@pytest.mark.parametrize("dtype", [C64, C128], ids=_ids)
@pytest.mark.parametrize("shape", [(16, 16, 16), (4, 6, 8)], ids=_ids)
def test_generator_numpy_backend_against_the_oracle(shape, dtype):
    gen = numpy_generator(shape, dtype)
    rms, pot = gen.delta_field_rms, np.array(gen.potential)
    check_generator_against_oracle(gen, shape, dtype)
    assert gen.delta_field_rms == rms and np.array_equal(gen.potential, pot)
    fz = 1.0 + 0.25 * np.arange(shape[2])
    got = gen.calculate_displacement_field("y", order=2, scale=-2.0, factor_z=fz).copy()
    plain = gen.calculate_displacement_field(1, order=2).copy()
    # scale enters squared, the table per plane: two transforms of the same phi2, each held to TOL rms
    assert np.max(np.abs(got - 4.0 * plain * fz)) <= 2 * TOL[dtype] * 4.0 * fz.max() * float(np.std(plain))


def test_generator_orders_and_light_cone():
    from randomfield_amd import Generator
    shape = (4, 6, 8)
    gen = numpy_generator(shape, C64)
    first = gen.calculate_displacement_field(0).copy()
    assert np.array_equal(gen.calculate_displacement_field(0, order=1), first)
    gen.calculate_displacement_field(2, order=2)
    assert np.array_equal(gen.calculate_displacement_field(0), first)          # order 1 is untouched by the second-order calls
    for bad in (0, 3, "2"):
        with pytest.raises(ValueError, match="order"):
            gen.calculate_displacement_field(0, order=bad)
    with pytest.raises(RuntimeError):                                            # light_cone needs the growth table
        gen.calculate_displacement_field(0, light_cone=True, order=2)
    g = 1.0 + 0.25 * np.arange(shape[2])
    grown = Generator(*shape, SPACING, backend="numpy", growth_function=g, mean_matter_density=np.ones(shape[2]))
    grown.generate_delta_field(seed=11, save_potential=True)
    want = grown.calculate_displacement_field(2, order=2).copy() * g * g
    assert np.allclose(grown.calculate_displacement_field(2, light_cone=True, order=2), want, rtol=1e-6, atol=0)
    grown.generate_delta_field(seed=11, save_potential=False)
    with pytest.raises(RuntimeError, match="No saved potential field."):
        grown.calculate_displacement_field("z", order=2)
    with pytest.raises(RuntimeError, match="No saved potential field."):
        grown.lpt2_source()


@pytest.mark.parametrize("dtype", [C64, C128], ids=_ids)
def test_generator_closed_forms_through_an_uploaded_potential(dtype):
    shape = (16, 16, 16)
    two, closed = orc.two_wave_potential(shape, SPACING, 1.5, -0.7, 2, 3, 0.3, 0.5)
    gen = numpy_generator(shape, dtype, potential=two)
    H = orc.hessian_fields(two, shape, SPACING)
    err = np.abs(gen.lpt2_source().astype(np.float64) - closed)
    assert np.all(err <= source_bound(H, dtype) + 1e-14)
    wave = orc.oblique_wave_potential(shape, SPACING, 2.0, (1, 2, 3))
    gen = numpy_generator(shape, dtype, potential=wave)
    H = orc.hessian_fields(wave, shape, SPACING)
    S = gen.lpt2_source()
    assert np.all(np.abs(S) <= source_bound(H, dtype))
    assert np.max(orc.source_magnitude(H)) > 0


def test_generator_divergence_identity():
    """sum_a D_a psi2_a = -(3/7) irfftn(S(k) k_dropped^2 / k^2) for the Generator's own S.  Every component is held to 2 TOL rms_a
    pointwise, hence to that in the rms norm, and D_a multiplies an rms by at most max |k_a|: the bound below, in the rms norm."""
    shape, dtype = (16, 16, 16), C128
    gen = numpy_generator(shape, dtype)
    S = gen.lpt2_source().copy()
    psi = [gen.calculate_displacement_field(a, order=2).copy() for a in range(3)]
    k2 = orc.ksq_grid(shape, SPACING)
    k2[0, 0, 0] = 1.0
    want = -(3.0 / 7.0) * orc.irfftn(orc.rfftn(S) * orc.dropped_ksq(shape, SPACING) / k2, shape)
    dk = orc.dk_of(shape, SPACING)
    bound = sum(dk[a] * np.max(np.abs(orc.modes(shape, a))) * 2 * TOL[dtype] * float(np.std(psi[a])) for a in range(3))
    err = float(np.sqrt(np.mean((orc.divergence(psi, shape, SPACING) - want) ** 2)))
    print("divergence: rms err / bound = %.3g" % (err / bound))
    assert err <= bound


def test_a_new_field_drops_the_cached_second_order_potential():
    shape, dtype = (4, 6, 8), C64
    gen = numpy_generator(shape, dtype, seed=11)
    a = gen.calculate_displacement_field(0, order=2).copy()
    assert np.array_equal(gen.calculate_displacement_field(0, order=2), a)      # (from the cache)
    gen.generate_delta_field(seed=12, save_potential=True)
    b = gen.calculate_displacement_field(0, order=2).copy()
    assert not np.array_equal(a, b)
    H = orc.hessian_fields(np.asarray(gen.potential, C128), shape, SPACING)     # the new field's potential
    S = gen.lpt2_source().copy()
    assert np.all(np.abs(S.astype(np.float64) - orc.source_from(H)) <= source_bound(H, dtype))
    own = orc.displacement2_from_source(S, shape, SPACING, 0)
    assert np.max(np.abs(b - own)) <= 2 * TOL[dtype] * float(np.std(own))
    assert np.max(np.abs(a - own)) > 2 * TOL[dtype] * float(np.std(own))        # ... which the old field's component is not


def test_abi_reports_lpt2():
    import os
    from randomfield_amd import _hip
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) == (5, 5) and _hip.abi_version() == (5, 5)
    assert _hip.FEATURES["lpt2"] == 1 << 16
    lib = _hip.load()
    assert lib.rf_version() == (5 << 16) | 5
    assert lib.rf_abi_features() & (1 << 16)
    assert "lpt2" in _hip.abi_features()
    assert _hip.RF_GRAD_FROM_POTENTIAL2 == 2
    for name in ("load_hessian", "execute_hessian", "lpt2_source", "lpt2_potential"):
        assert hasattr(_hip.DevicePlan, name)
    for name in ("rf_load_hessian", "rf_execute_hessian_c2r", "rf_lpt2_source", "rf_lpt2_potential"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    header = open(os.path.join(emu_util.ROOT, "include", "randomfield_hip.h")).read()
    assert "RF_FEATURE_LPT2 = 1 << 16" in header and "RF_GRAD_FROM_POTENTIAL2 = 2" in header
    assert "#define RF_ABI_MAJOR 5" in header and "#define RF_ABI_MINOR 5" in header
