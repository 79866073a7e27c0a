"""The gradient of the saved potential, psi_a(k) = i k_a delta(k) / k^2 (csrc/rf_core.h grad_cell), on the CPU emulator: the cell function
over an array from both sources (emu_gradient_k, the elementwise kernel's loop), the generic sequence that applies it inside the x pass
(rf_generic.h generic_c2r_from_seq, GenericDerivSource) against "elementwise, then generic_c2r_seq" bit for bit, the float64 oracle
np.fft.irfftn(1j * k_a * Phat), the divergence identity, the numpy backend of Generator.calculate_displacement_field and the ABI
surface (5.5, feature bit 14).  No GPU needed.

Tolerances.  Elementwise: the function rounds twice (the factor, then the product), which bounds the relative error of a component
near 1 eps; 4 eps is the margin.  Fields: 1e-5 * rms (float32) and 1e-11 * rms (float64), the generic path's own tolerances
(tests/test_gpu_generic.py), on the maximum absolute error."""
import ctypes

import numpy as np
import pytest

import emu_util
from randomfield_amd import powertools, transform

SPACING = 2.5
C64, C128 = np.complex64, np.complex128
K_SHAPES = [(4, 6, 8), (6, 4, 12), (16, 16, 16)]
SEQ_SHAPES = [(4, 6, 8), (40, 60, 80), (30, 14, 22)]
TOL = {C64: 1e-5, C128: 1e-11}

_c_dp = ctypes.POINTER(ctypes.c_double)
_HEAD = [ctypes.c_int] * 5 + [ctypes.c_double, ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_dp, ctypes.c_void_p, ctypes.c_longlong]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else ("c64" if v == C64 else "c128")


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_gradient_k.argtypes = _HEAD + [ctypes.c_void_p]
    lib.emu_gradient_k.restype = ctypes.c_int
    lib.emu_generic_gradient_c2r.argtypes = _HEAD + [ctypes.c_void_p, _c_dp, _c_dp]
    lib.emu_generic_gradient_c2r.restype = ctypes.c_int
    return lib


def spectrum(shape, dtype, seed=3):
    """a random half spectrum, Hermitian-symmetrised as the generator's (transform.py:141-158)"""
    nx, ny, nz = shape
    rng = np.random.RandomState(seed)
    data = (rng.normal(size=(nx, ny, nz // 2 + 1)) + 1j * rng.normal(size=(nx, ny, nz // 2 + 1))).astype(dtype)
    if (nz // 2 + 1) % 2:
        transform.symmetrize(data, packed=True)
    else:
        # (transform.symmetrize takes an odd number of stored planes, nz a multiple of 4, as the reference's: the same symmetry by
        # averaging the kz = 0 and nz/2 planes with their mirrored conjugates)
        for kz in (0, nz // 2):
            plane = data[:, :, kz]
            mirror = np.conj(np.roll(plane[::-1, ::-1], (1, 1), axis=(0, 1)))
            data[:, :, kz] = 0.5 * (plane + mirror)
        data[0, 0, 0] = 0
    return data


def ksq(shape):
    return tuple(np.ascontiguousarray(a, np.float64) for a in powertools.ksq_axes(*shape, SPACING))


def dk_of(shape, axis):
    return 2 * np.pi / (shape[axis] * SPACING)


def k_axis(shape, axis):
    """k_a of every cell along `axis` (broadcastable over the half spectrum), the axis' Nyquist entry set to 0"""
    n = shape[axis]
    k = 2 * np.pi * (np.fft.rfftfreq(n, SPACING) if axis == 2 else np.fft.fftfreq(n, SPACING))
    k[n // 2] = 0.0
    return k.reshape([-1 if a == axis else 1 for a in range(3)])


def ksq_grid(shape):
    kx2, ky2, kz2 = ksq(shape)
    return (kx2[:, None, None] + ky2[None, :, None]) + kz2[None, None, :]


def want_k(src, shape, axis, scale, divide):
    """float64 formula on the same input"""
    out = 1j * scale * k_axis(shape, axis) * src.astype(C128)
    if divide:
        k2 = ksq_grid(shape)
        k2[0, 0, 0] = 1.0
        out = out / k2
        out[0, 0, 0] = 0.0
    return out


def _args(shape, dtype, axis, scale, divide, src, pitch=None):
    nx, ny, nz = shape
    kx2, ky2, kz2 = ksq(shape)
    keep = (kx2, ky2, kz2, src)
    pitch = nz // 2 + 1 if pitch is None else pitch
    return (int(dtype == C128), nx, ny, nz, axis, float(scale), dk_of(shape, axis), int(divide), emu_util._dp(kx2), emu_util._dp(ky2),
            emu_util._dp(kz2), src.ctypes.data_as(ctypes.c_void_p), pitch), keep


def gradient_k(lib, src, shape, axis, scale, divide, pitch=None):
    args, keep = _args(shape, src.dtype.type, axis, scale, divide, src, pitch)
    nx, ny, nz = shape
    out = np.empty((nx, ny, nz // 2 + 1), src.dtype)
    assert lib.emu_gradient_k(*args, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def gradient_field(lib, src, shape, axis, scale, divide, pitch=None):
    args, keep = _args(shape, src.dtype.type, axis, scale, divide, src, pitch)
    out = np.empty(shape, np.float32 if src.dtype == C64 else np.float64)
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    assert lib.emu_generic_gradient_c2r(*args, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(s1), ctypes.byref(s2)) == 0
    return out, s1.value, s2.value


def assert_elementwise(got, want, dtype):
    eps = np.finfo(np.float32 if dtype == C64 else np.float64).eps
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        err, bound = np.abs(g.astype(np.float64) - w), 4 * eps * np.abs(w)
        print("elementwise: max err / (eps |want|) = %.3f" % np.max(err[w != 0] / (eps * np.abs(w[w != 0]))))
        assert np.all(err <= bound)
        assert np.all(g[w == 0] == 0)


def zero_planes(shape, axis):
    """index of the cells the rule makes exactly zero: the planes m = 0 of the axis (index 0 and the Nyquist index)"""
    sel = [slice(None)] * 3
    sel[axis] = [0, shape[axis] // 2]
    return tuple(sel)


@pytest.mark.parametrize("dtype", [C64, C128], ids=_ids)
@pytest.mark.parametrize("shape", K_SHAPES, ids=_ids)
def test_gradient_k_elementwise_both_sources(lib, shape, dtype):
    src = spectrum(shape, dtype)
    scale = -1.75
    for axis in range(3):
        for divide in (0, 1):
            got = gradient_k(lib, src, shape, axis, scale, divide)
            assert_elementwise(got, want_k(src, shape, axis, scale, divide), dtype)
            assert transform.is_hermitian(got, packed=True)
            assert np.all(got[zero_planes(shape, axis)] == 0) and got[0, 0, 0] == 0
            assert float(np.abs(got).max()) > 0


def test_gradient_k_reads_a_padded_source_and_works_in_place(lib):
    """the stored potential's rows are padded (float32 plans: an even pitch); K in place is the divide mode's form"""
    shape = (6, 4, 12)
    src = spectrum(shape, C64)
    padded = np.full((6, 4, 10), np.nan + 0j, C64)
    padded[:, :, :7] = src
    assert np.array_equal(gradient_k(lib, padded, shape, 1, 2.0, 0, pitch=10), gradient_k(lib, src, shape, 1, 2.0, 0))
    want = gradient_k(lib, src, shape, 0, 1.0, 1)
    args, keep = _args(shape, C64, 0, 1.0, 1, src)
    assert lib.emu_gradient_k(*args, src.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(src, want)


@pytest.mark.parametrize("dtype", [C64, C128], ids=_ids)
@pytest.mark.parametrize("shape", SEQ_SHAPES, ids=_ids)
def test_fused_sequence_equals_elementwise_then_c2r_bit_for_bit(lib, shape, dtype):
    src = spectrum(shape, dtype)
    k2 = ksq_grid(shape)
    k2[0, 0, 0] = 1.0
    pot = (src / k2).astype(dtype)
    pot[0, 0, 0] = 0
    rt = np.float32 if dtype == C64 else np.float64
    for axis in range(3):
        for divide, source in ((0, pot), (1, src)):
            oracle = np.fft.irfftn(want_k(source, shape, axis, 1.0, divide), s=shape, axes=(0, 1, 2))
            rms = float(np.std(oracle))
            assert rms > 0
            for walk in (None, (16, 16)):
                if walk is None:
                    want, w1, w2 = emu_util.generic_c2r(gradient_k(lib, source, shape, axis, 1.0, divide))
                    got, g1, g2 = gradient_field(lib, source, shape, axis, 1.0, divide)
                else:
                    with emu_util.generic_threads(*walk):
                        want, w1, w2 = emu_util.generic_c2r(gradient_k(lib, source, shape, axis, 1.0, divide))
                        got, g1, g2 = gradient_field(lib, source, shape, axis, 1.0, divide)
                assert got.dtype == rt and np.array_equal(got, want), (axis, divide, walk)
                assert (g1, g2) == (w1, w2)
                err = float(np.max(np.abs(got - oracle)))
                print("field: axis %d divide %d walk %s max err / rms = %.3g" % (axis, divide, walk, err / rms))
                assert err <= TOL[dtype] * rms
    # a padded source through the fused x pass too
    nzh = shape[2] // 2 + 1
    padded = np.zeros(shape[:2] + (nzh + 2,), dtype)
    padded[:, :, :nzh] = pot
    assert np.array_equal(gradient_field(lib, padded, shape, 0, 1.0, 0, pitch=nzh + 2)[0], gradient_field(lib, pot, shape, 0, 1.0, 0)[0])


def test_split_x_axis_takes_the_unfused_fallback(lib):
    """an x axis in the four-step form: the component goes into scratch and the ordinary passes run from there"""
    shape = (40, 60, 80)
    pot = spectrum(shape, C64)
    old = lib.emu_set_generic_cap(16)
    try:
        want = emu_util.generic_c2r(gradient_k(lib, pot, shape, 0, 1.0, 0))[0]
        got = gradient_field(lib, pot, shape, 0, 1.0, 0)[0]
    finally:
        lib.emu_set_generic_cap(old)
    assert np.array_equal(got, want)
    plain = gradient_field(lib, pot, shape, 0, 1.0, 0)[0]
    assert not np.array_equal(got, plain) and np.max(np.abs(got - plain)) <= 1e-5 * float(np.std(plain))


def test_divergence_of_the_vector_field_is_minus_delta(lib):
    """sum_a d psi_a / d x_a = -delta, spectral derivatives, once the k-space Nyquist planes of delta are zero (there i k drops the mode)"""
    shape = (16, 16, 16)
    delta_k = spectrum(shape, C128)
    delta_k[8, :, :] = 0
    delta_k[:, 8, :] = 0
    delta_k[:, :, 8] = 0
    delta_k[0, 0, 0] = 0
    delta = np.fft.irfftn(delta_k, s=shape, axes=(0, 1, 2))
    div = np.zeros(shape)
    for axis in range(3):
        psi = gradient_field(lib, delta_k, shape, axis, 1.0, 1)[0]
        div += np.fft.irfftn(1j * k_axis(shape, axis) * np.fft.rfftn(psi, axes=(0, 1, 2)), s=shape, axes=(0, 1, 2))
    err = float(np.max(np.abs(div + delta)))
    print("divergence: max err / rms = %.3g" % (err / np.std(delta)))
    assert err <= 1e-11 * float(np.std(delta))


def test_generator_numpy_backend():
    from randomfield_amd import Generator
    shape = (4, 6, 8)
    gen = Generator(*shape, SPACING, backend="numpy")
    with pytest.raises(RuntimeError, match="No saved potential field."):
        gen.calculate_displacement_field(0)
    gen.generate_delta_field(seed=11, save_potential=True)
    rms = gen.delta_field_rms
    pot = gen.potential.astype(C128)
    fz = 1.0 + 0.25 * np.arange(shape[2])
    for axis, name in enumerate("xyz"):
        oracle = np.fft.irfftn(1j * k_axis(shape, axis) * pot, s=shape, axes=(0, 1, 2))
        tol = 1e-5 * float(np.std(oracle))
        got = gen.calculate_displacement_field(axis).copy()
        assert got.shape == shape and np.max(np.abs(got - oracle)) <= tol
        assert np.array_equal(gen.calculate_displacement_field(name), got)
        scaled = gen.calculate_displacement_field(axis, scale=-2.0, factor_z=fz).copy()
        assert np.max(np.abs(scaled - (-2.0) * oracle * fz)) <= 2 * fz.max() * tol
    assert gen.delta_field_rms == rms and np.array_equal(gen.potential.astype(C128), pot)
    with pytest.raises(ValueError):
        gen.calculate_displacement_field(3)
    with pytest.raises(RuntimeError):                      # light_cone needs the growth table
        gen.calculate_displacement_field(0, light_cone=True)
    grown = Generator(*shape, SPACING, backend="numpy", growth_function=fz, mean_matter_density=np.ones(shape[2]))
    grown.generate_delta_field(seed=11, save_potential=True)
    want = grown.calculate_displacement_field(2).copy() * fz
    assert np.allclose(grown.calculate_displacement_field(2, light_cone=True), want, rtol=1e-6, atol=0)
    grown.generate_delta_field(seed=11, save_potential=False)
    with pytest.raises(RuntimeError, match="No saved potential field."):
        grown.calculate_displacement_field("z")


def test_abi_reports_the_gradient():
    from randomfield_amd import _hip
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) == (5, 5) and _hip.abi_version() == (5, 5)
    assert _hip.FEATURES["gradient"] == 1 << 14
    lib = _hip.load()
    assert lib.rf_version() == (5 << 16) | 5
    assert lib.rf_abi_features() & (1 << 14)
    assert "gradient" in _hip.abi_features()
    assert (_hip.RF_GRAD_FROM_POTENTIAL, _hip.RF_GRAD_FROM_KSPACE) == (0, 1)
    assert hasattr(_hip.DevicePlan, "load_gradient") and hasattr(_hip.DevicePlan, "execute_gradient")
